"""NumPy oracle of morig_amd/transfer.py (csrc/transfer.hip, csrc/pointtri_core.h), float64 without fused
multiply-adds, every operation in the order the kernels and the header state.

Part A  ``remesh_loop``: the reference's transfer_rig_to_remesh (data_proc/common_ops.py:229-259) replayed line for line -- the sweeps,
        the ascending visit, the strict ``<`` from 1e8 over the ascending neighbours -- with three differences that change no result the
        reference delivers: distances are taken per pair where the loop needs them (``np.sqrt(np.sum(d ** 2, -1))`` of three terms is
        ``sqrt((dx dx + dy dy) + dz dz)``) instead of from two dense matrices; the neighbour sets, which do not change between the sweeps,
        are built once (``neighbour_sets``; ``neighbours_by_argwhere`` is the reference's own expression, and the tests hold one against the
        other); a sweep that fills nothing ends the loop, where the reference spins forever. A corner position c with no face number c
        (fewer than three faces) adds nothing, where the reference's indexing raises IndexError. ``remesh_parallel`` is the parallel form
        the kernel runs.
Part B  ``closest`` / ``transfer_skins``: the seven regions of pointtri_core.h for all (point, triangle) pairs at once, elementwise in the
        header's order of operations."""
import numpy as np

INF_SWEEP = -1
REGIONS = ("vertex_a", "vertex_b", "edge_ab", "vertex_c", "edge_ac", "edge_bc", "face")


# ------------------------------------------------------------------------------------------------------------------------- part A
def dist2(p, q):
    d = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def coincide(vr, vo):
    """-> (coincident int64 [V']: the lowest original vertex at squared distance 0 or -1 (np.argmin of a row whose minimum is 0),
    nearest int64 [V']: np.argmin of the squared distances or -1 without originals)"""
    vr, vo = np.asarray(vr, dtype=np.float64).reshape(-1, 3), np.asarray(vo, dtype=np.float64).reshape(-1, 3)
    coin, near = np.full(len(vr), -1, dtype=np.int64), np.full(len(vr), -1, dtype=np.int64)
    if len(vo) == 0:
        return coin, near
    for s in range(0, len(vr), 512):
        with np.errstate(all="ignore"):
            d = dist2(vr[s:s + 512, None, :], vo[None, :, :])
        near[s:s + 512] = np.argmin(d, 1)
        zero = d == 0.0
        coin[s:s + 512] = np.where(zero.any(1), np.argmax(zero, 1), -1)
    return coin, near


def neighbours_by_argwhere(faces, v):
    """the reference's expression (common_ops.py:243-244)"""
    ids = np.unique(faces[np.argwhere(faces == v)])
    return np.delete(ids, np.where(ids == v))


def neighbour_sets(faces, n_verts, mode):
    """per vertex the ascending neighbour ids. "faces": the vertices of the faces that contain v. "reference": also the vertices of face
    number c for every corner position c at which v stands (what indexing ``faces`` with both columns of argwhere yields)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    sets = [set() for _ in range(n_verts)]
    for row in faces:
        for c in range(3):
            sets[row[c]].update(int(x) for x in row)
            if mode == "reference" and c < len(faces):
                sets[row[c]].update(int(x) for x in faces[c])
    return [np.array(sorted(s - {v}), dtype=np.int64) for v, s in enumerate(sets)]


def remesh_loop(vo, vr, faces, skins, neighbours="reference", unreachable="raise"):
    """-> dict(source int64 [V'] (-1: never filled), sweep int64 [V'] (0 coincident, k filled in sweep k, -1 never), skins [V', J],
    n_sweeps, n_unreachable). ``unreachable="nearest"`` gives a vertex no sweep fills its nearest original vertex."""
    vo, vr = np.asarray(vo, dtype=np.float64).reshape(-1, 3), np.asarray(vr, dtype=np.float64).reshape(-1, 3)
    skins = np.asarray(skins, dtype=np.float64)
    coin, near = coincide(vr, vo)
    nbrs = neighbour_sets(faces, len(vr), neighbours)
    filled_flag = coin >= 0
    source, sweep = coin.copy(), np.where(filled_flag, 0, INF_SWEEP).astype(np.int64)
    n_sweeps = 0
    while not np.all(filled_flag):
        unfilled_pos = np.argwhere(filled_flag == False).squeeze(axis=1)       # noqa: E712  (the reference's line)
        n_sweeps += 1
        progress = False
        for v in unfilled_pos:
            neighbor_ids = nbrs[v]
            if filled_flag[neighbor_ids].sum() > 0:
                closest_nn = -1
                closest_dist = 1e8
                for nv in neighbor_ids:
                    if filled_flag[nv]:
                        d = np.sqrt(dist2(vr[v], vr[nv]))
                        if d < closest_dist:
                            closest_dist = d
                            closest_nn = nv
                source[v] = source[closest_nn]
                filled_flag[v] = True
                sweep[v] = n_sweeps
                progress = True
        if not progress:
            n_sweeps -= 1
            break
    lost = ~filled_flag
    if unreachable == "nearest":
        source[lost] = near[lost]
    return dict(source=source, sweep=sweep, skins=gather_rows(skins, source), n_sweeps=n_sweeps, n_unreachable=int((source < 0).sum()),
                coincident=coin, nearest=near)


def ascending_sum(x):
    s = np.zeros(x.shape[0])
    for j in range(x.shape[1]):
        s = s + x[:, j]
    return s


def normalise_rows(rows):
    with np.errstate(all="ignore"):
        return rows / (ascending_sum(rows) + 1e-8)[:, None]


def gather_rows(skins, source):
    skins = np.asarray(skins, dtype=np.float64)
    out = np.zeros((len(source), skins.shape[1]))
    won = source >= 0
    if won.any():
        out[won] = normalise_rows(skins[source[won]])
    return out


def remesh_parallel(vo, vr, faces, neighbours="reference"):
    """the parallel form: fill times as the fixed point of T[v] = min_u T[u] + (T[u] == 0 or u > v), parents, pointer chasing
    -> (source, sweep)"""
    vr = np.asarray(vr, dtype=np.float64).reshape(-1, 3)
    coin, _ = coincide(vr, vo)
    nbrs = neighbour_sets(faces, len(vr), neighbours)
    BIG = 1 << 40
    T = np.where(coin >= 0, 0, BIG).astype(np.int64)
    changed = True
    while changed:
        changed = False
        for v in range(len(vr) - 1, -1, -1):                                   # any order ends in the same fixed point: the worst one here
            if T[v] == 0:
                continue
            for u in nbrs[v]:
                if T[u] < BIG:
                    cand = T[u] + (1 if (T[u] == 0 or u > v) else 0)
                    if cand < T[v]:
                        T[v], changed = cand, True
    parent = np.arange(len(vr))
    for v in range(len(vr)):
        if T[v] == 0 or T[v] == BIG:
            continue
        best, nn = 1e8, -1
        for u in nbrs[v]:
            if T[u] == 0 or T[u] < T[v] or (T[u] == T[v] and u < v):
                d = np.sqrt(dist2(vr[v], vr[u]))
                if d < best:
                    best, nn = d, u
        parent[v] = nn
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            break
        parent = nxt
    source = np.where(T[parent] == 0, coin[parent], -1)
    return source, np.where(T == BIG, INF_SWEEP, T)


# ------------------------------------------------------------------------------------------------------------------------- part B
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest(points, tri):
    """points [P, 3], tri [F, 3, 3] -> (region int [P, F], bary [P, F, 3], d2 [P, F]) by pointtri_core.h"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 1, 3)
    tri = np.asarray(tri, dtype=np.float64).reshape(1, -1, 3, 3)
    a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        v_ab, w_ac, w_bc = d1 / (d1 - d3), d2 / (d2 - d6), e43 / (e43 + e56)
        s = (va + vb) + vc
        v_f, w_f = vb / s, vc / s
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        barys = [(one, zero, zero), (zero, one, zero), (1.0 - v_ab, v_ab, zero), (zero, zero, one), (1.0 - w_ac, zero, w_ac),
                 (zero, 1.0 - w_bc, w_bc), ((1.0 - v_f) - w_f, v_f, w_f)]
        region = np.full(d1.shape, 6, dtype=np.int64)
        bary = np.stack(barys[6], -1)
        for k in range(5, -1, -1):                                             # the first condition that holds decides
            region = np.where(conds[k], k, region)
            bary = np.where(conds[k][..., None], np.stack(barys[k], -1), bary)
        q = (bary[..., 0:1] * a + bary[..., 1:2] * b) + bary[..., 2:3] * c
        dist = dist2(p, q)
    return region, bary, dist


def closest_face(points, verts, faces, chunk=256):
    """-> (face int32 [P] (-1), bary [P, 3] (NaN), distance [P] (NaN), region int [P] (-1)): the smallest squared distance under a strict
    ``<`` from +inf over ascending faces"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    P = len(points)
    face, bary = np.full(P, -1, dtype=np.int32), np.full((P, 3), np.nan)
    dist, region = np.full(P, np.nan), np.full(P, -1, dtype=np.int64)
    if len(faces) == 0 or P == 0:
        return face, bary, dist, region
    tri = np.asarray(verts, dtype=np.float64).reshape(-1, 3)[faces]
    for s in range(0, P, chunk):
        r, b, d = closest(points[s:s + chunk], tri)
        d = np.where(np.isnan(d), np.inf, d)
        k = np.argmin(d, 1)
        rows = np.arange(len(k))
        won = d[rows, k] < np.inf
        face[s:s + chunk] = np.where(won, k, -1)
        bary[s:s + chunk] = np.where(won[:, None], b[rows, k], np.nan)
        dist[s:s + chunk] = np.where(won, np.sqrt(d[rows, k]), np.nan)
        region[s:s + chunk] = np.where(won, r[rows, k], -1)
    return face, bary, dist, region


def blend_rows(skins, faces, face, bary):
    skins = np.asarray(skins, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    J = skins.shape[1]
    out = np.zeros((len(face), J))
    won = face >= 0
    if won.any():
        f, b = faces[face[won]], bary[won]
        with np.errstate(all="ignore"):
            rows = (b[:, 0:1] * skins[f[:, 0]] + b[:, 1:2] * skins[f[:, 1]]) + b[:, 2:3] * skins[f[:, 2]]
        out[won] = normalise_rows(rows)
    return out


def transfer_skins(src_verts, src_faces, src_skins, dst_verts):
    face, bary, dist, region = closest_face(dst_verts, src_verts, src_faces)
    return dict(skins=blend_rows(src_skins, src_faces, face, bary), face=face, bary=bary, distance=dist, region=region)


# ------------------------------------------------------------------------------------------------------------------------- generators
class PlainRig:
    """what transfer_to_remesh needs of a rig: ``skins`` (and whatever else, copied along)"""

    def __init__(self, skins, pos=None, hierarchy=None):
        self.skins = np.asarray(skins, dtype=np.float64)
        J = self.skins.shape[1]
        self.pos = np.zeros((J, 3)) if pos is None else np.asarray(pos, dtype=np.float64)
        self.hierarchy = np.array([-1] + [0] * (J - 1)) if hierarchy is None else np.asarray(hierarchy)


def grid_mesh(nx, ny, seed=None, step=0.125):
    """an nx x ny vertex grid in the plane z = 0 on a binary grid, two faces per cell; ``seed``: vertices renumbered at random"""
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    verts = np.stack([ii.ravel() * step, jj.ravel() * step, np.zeros(nx * ny)], 1)
    idx = lambda i, j: i * ny + j
    faces = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            faces += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    faces = np.array(faces, dtype=np.int64).reshape(-1, 3)
    if seed is not None:
        rng = np.random.default_rng(seed)
        perm = rng.permutation(len(verts))                                     # new id of old vertex k
        inv = np.argsort(perm)
        verts, faces = verts[inv], perm[faces]
        faces = faces[rng.permutation(len(faces))]
    return verts, faces


def chain_mesh(n, descending=False, step=0.125):
    """n vertices on a line joined by the faces (k, k + 1, k + 1): under "faces" vertex k neighbours k - 1 and k + 1 only. With the one
    coincident vertex at the start of the line, ``descending`` numbers the vertices from the far end: a sweep, visiting in ascending
    index, then fills ONE vertex, and the flood needs n - 1 sweeps; ascending numbering needs one."""
    k = np.arange(n)
    verts = np.stack([k * step, np.zeros(n), np.zeros(n)], 1)
    faces = np.stack([k[:-1], k[1:], k[1:]], 1).astype(np.int64)
    if descending:
        verts, faces = verts[::-1].copy(), (n - 1 - faces)
    return verts, faces


def chain_case(n, descending, J=3):
    """-> (vo, vr, faces, skins): the chain with ONE original vertex, at the start of the line"""
    vr, faces = chain_mesh(n, descending)
    start = n - 1 if descending else 0
    return vr[start:start + 1].copy(), vr, faces, random_skins(1, J, n)


def torus(nu, nv, R=0.5, r=0.2):
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), r * np.sin(v), (R + r * np.cos(v)) * np.sin(u)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = []
    for i in range(nu):
        for j in range(nv):
            faces += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return verts, np.array(faces, dtype=np.int64)


def random_skins(n, J, seed):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 1, (n, J)) * (rng.uniform(0, 1, (n, J)) < 0.4)
    s[np.arange(n), rng.integers(0, J, n)] += 0.25
    return s / s.sum(1, keepdims=True)


def remesh_case(nx, ny, keep_every, seed, J=5):
    """a shuffled grid as the remeshed mesh; the originals are every ``keep_every``-th of its vertices plus a few elsewhere"""
    vr, faces = grid_mesh(nx, ny, seed)
    rng = np.random.default_rng(seed + 1)
    pick = np.sort(rng.permutation(len(vr))[:max(len(vr) // keep_every, 1)])
    vo = np.concatenate([vr[pick], rng.uniform(2, 3, (3, 3))])[rng.permutation(len(pick) + 3)]
    return vo, vr, faces, random_skins(len(vo), J, seed + 2)


def root_tie_case():
    """vertex 2 at the origin between the filled vertices 0 at squared distance 1 + 2^-52 and 1 at squared distance 1: both roots round to
    1.0, so the strict ``<`` keeps vertex 0 although its square is the larger one -> source[2] = 0. The face stands three times: the
    reference indexes face NUMBERS 0, 1, 2."""
    vr = np.array([[1.0, 2.0 ** -26, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    return vr[:2].copy(), vr, np.array([[0, 1, 2]] * 3, dtype=np.int64), np.array([[0.75, 0.25], [0.125, 0.875]])


def underflow_case():
    """remeshed vertex 0 differs from original 1 by 1e-170 in x (its square underflows to 0) and by the sign of a zero in z; original 2
    coincides with it exactly: the lowest, 1, gives the row"""
    vo = np.array([[1.0, 1.0, 1.0], [1e-170, 0.25, -0.0], [0.0, 0.25, 0.0]])
    vr = np.array([[0.0, 0.25, 0.0], [0.125, 0.25, 0.0], [0.0, 0.5, 0.0]])
    return vo, vr, np.array([[0, 1, 2]] * 3, dtype=np.int64), np.array([[0.5, 0.5, 0.0], [0.25, 0.0, 0.75], [0.0, 1.0, 0.0]])


# the seven regions on a binary grid: triangle a = (0, 0, 0), b = (1, 0, 0), c = (0, 1, 0); every product is exact
REGION_TRIANGLE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
REGION_POINTS = [  # point, region, bary, squared distance
    ([-0.5, -0.25, 0.5], "vertex_a", [1.0, 0.0, 0.0], 0.5625),
    ([1.5, -0.25, 0.0], "vertex_b", [0.0, 1.0, 0.0], 0.3125),
    ([0.25, -0.5, 0.25], "edge_ab", [0.75, 0.25, 0.0], 0.3125),
    ([-0.25, 1.5, 0.0], "vertex_c", [0.0, 0.0, 1.0], 0.3125),
    ([-0.5, 0.75, 0.0], "edge_ac", [0.25, 0.0, 0.75], 0.25),
    ([1.0, 1.0, 0.0], "edge_bc", [0.0, 0.5, 0.5], 0.5),
    ([0.25, 0.25, 0.5], "face", [0.5, 0.25, 0.25], 0.25),
]
# a zero-area triangle, a = (0, 0, 0), b = (1, 0, 0), c = (2, 0, 0) on one line: va = vb = vc = 0 and the vertex and edge comparisons decide
DEGENERATE_TRIANGLE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
DEGENERATE_POINTS = [([-1.0, 1.0, 0.0], "vertex_a", [1.0, 0.0, 0.0], 2.0), ([0.5, 0.5, 0.0], "edge_ab", [0.5, 0.5, 0.0], 0.25),
                     ([1.5, 0.5, 0.0], "edge_ac", [0.25, 0.0, 0.75], 0.25), ([3.0, 0.0, 1.0], "vertex_c", [0.0, 0.0, 1.0], 2.0)]
# two corners in one place, a = b: the edge (a, b) has no length and its quotient is 0 / 0; that triangle's distance is then no number and
# loses every ``<``, so the neighbouring triangle (a, c, d), which shares the corners, gives the answer
COLLAPSED_VERTS = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
COLLAPSED_FACES = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
COLLAPSED_POINT = [0.25, -0.5, 0.0]                                            # -> face 1, its edge (a, b) = (0, 2): bary (0.75, 0.25, 0)
# two triangles sharing the edge (0,0,0)-(1,0,0) in the planes z = 0: a point above the edge's middle is equally far from both
TIE_VERTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
TIE_FACES = np.array([[0, 3, 1], [0, 1, 2]], dtype=np.int64)
TIE_POINT = [0.5, 0.0, 0.25]                                                   # -> face 0, its edge (a, c) = (0, 1): bary (0.5, 0, 0.5)
