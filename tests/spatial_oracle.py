"""NumPy restatement of morig_amd/spatial.py and csrc/bvh.hip, for the CPU tests and as the reference of the GPU
tests. It holds the brute-force rules (the ray rule of tests/labels_oracle.py, the point rule of tests/transfer_oracle.py, both with the
kernels' clamping of a face index outside its mesh), the same tree -- Morton keys, stable order, exact boxes per level -- and the same
traversal rule as csrc/bvh_core.h, query by query, with the count of box and face tests. One mesh at a time; the batch is the callers'."""
import numpy as np

import labels_oracle as lo
import transfer_oracle as to

WIDTH, MAX_LEVELS, SLACK = 64, 4, 2.0 ** -40
BAD_FACE = 1


def clamped(verts, faces):
    """-> (faces with every index clamped into the mesh as the kernels clamp it (none left for a mesh without vertices), bad: bool)"""
    verts, faces = np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(faces) == 0:
        return faces, False
    if len(verts) == 0:
        return faces[:0], True
    bad = bool(faces.min() < 0 or faces.max() >= len(verts))
    return np.clip(faces, 0, len(verts) - 1), bad


# ------------------------------------------------------------------------------------------------------------------------- brute force
def brute_cast(origins, dirs, verts, faces, orientation=0):
    """-> dict(t, face, point, bad): morig_ray_cast on one mesh"""
    fc, bad = clamped(verts, faces)
    c = lo.cast(origins, dirs, verts, fc, orientation)
    return dict(t=c["t"], face=c["face"], point=c["point"], bad=bad and len(np.asarray(origins).reshape(-1, 3)) > 0)


def brute_closest(points, verts, faces):
    """-> dict(face, bary, distance, bad, no_faces): morig_transfer_closest on one mesh"""
    fc, bad = clamped(verts, faces)
    n = len(np.asarray(points).reshape(-1, 3))
    face, bary, dist, _ = to.closest_face(points, verts, fc)
    return dict(face=face, bary=bary, distance=dist, bad=bad and n > 0, no_faces=len(fc) == 0 and n > 0)


# ------------------------------------------------------------------------------------------------------------------------- the tree
def _spread10(v):
    v = v & 0x3ff
    v = (v | (v << 16)) & 0x030000ff
    v = (v | (v << 8)) & 0x0300f00f
    v = (v | (v << 4)) & 0x030c30c3
    v = (v | (v << 2)) & 0x09249249
    return v


def morton_codes(verts, faces):
    """the 30-bit code of every (clamped) face: bvh_core.h morton30 in the frame of the mesh's bounding box"""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    codes = np.zeros(len(faces), dtype=np.int64)
    if len(faces) == 0 or len(verts) == 0:
        return codes
    with np.errstate(all="ignore"):
        mn, mx = np.full(3, np.inf), np.full(3, -np.inf)
        for k in range(3):                                                              # morig_mesh_bbox: `<` and `>`, a NaN never enters
            col = verts[:, k]
            col = col[~np.isnan(col)]
            if len(col):
                mn[k], mx[k] = col.min(), col.max()
        ext = mx[0] - mn[0]
        for k in (1, 2):
            if mx[k] - mn[k] > ext:
                ext = mx[k] - mn[k]
        if not (ext > 0.0) or not np.isfinite(ext):
            return codes
        A, B, C = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
        c = ((A + B) + C) / 3.0
        q = (c - mn[None, :]) / ext * 1024.0
        cell = np.where(q >= 0.0, np.where(q >= 1023.0, 1023.0, np.floor(q)), 0.0)
        cell = np.where(np.isnan(cell), 0.0, cell).astype(np.int64)
        code = (_spread10(cell[:, 0]) << 2) | (_spread10(cell[:, 1]) << 1) | _spread10(cell[:, 2])
        return np.where(np.isfinite(c).all(1), code, 0)


def level_counts(n_faces):
    """the nodes of levels 1 .. of one mesh, up to the first level with one node ([] without faces)"""
    out, n = [], int(n_faces)
    while n > 0 and (not out or n > 1):
        n = (n + WIDTH - 1) // WIDTH
        out.append(n)
    assert len(out) <= MAX_LEVELS
    return out


def _group_boxes(boxes):
    n = (len(boxes) + WIDTH - 1) // WIDTH
    out = np.empty((n, 6))
    for i in range(n):
        part = boxes[i * WIDTH:(i + 1) * WIDTH]
        out[i, :3], out[i, 3:] = part[:, :3].min(0), part[:, 3:].max(0)                # +inf / -inf of the empty box are neutral
    return out


def build(verts, faces, order=None):
    """-> dict(verts, faces (clamped), bad, order int64 [F]: the face at every sorted position, levels: the boxes [n_k, 6] of level
    1, 2, ...). ``order``: keep this order instead of sorting (a refit)"""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    fc, bad = clamped(verts, faces)
    order = np.argsort(morton_codes(verts, fc), kind="stable") if order is None else np.asarray(order, dtype=np.int64)[:len(fc)]
    levels = []
    if len(fc):
        tri = verts[fc[order]]                                                          # [F, 3 corners, 3]
        boxes = np.concatenate([tri.min(1), tri.max(1)], 1)
        boxes[np.isnan(tri).any((1, 2))] = [np.inf] * 3 + [-np.inf] * 3
        for _ in level_counts(len(fc)):
            boxes = _group_boxes(boxes)
            levels.append(boxes)
        assert len(levels[-1]) == 1
    return dict(verts=verts, faces=fc, bad=bad, order=order, levels=levels)


# ------------------------------------------------------------------------------------------------------------------------- entering
def query_scale(q, root):
    s = 0.0
    with np.errstate(all="ignore"):
        for k in range(3):
            s = s + ((root[3 + k] - root[k]) + abs(q[k] - 0.5 * (root[k] + root[3 + k])))
    return s


def ray_skips(o, d, boxes, scale, best):
    """boxes [n, 6] -> (skip bool [n], bound [n]): bvh_core.h ray_skips"""
    n = len(boxes)
    with np.errstate(all="ignore"):
        pad = SLACK * scale
        tmin, tmax, missed = np.full(n, -np.inf), np.full(n, np.inf), np.zeros(n, dtype=bool)
        for k in range(3):
            a, b = (boxes[:, k] - pad) - o[k], (boxes[:, 3 + k] + pad) - o[k]
            if d[k] == 0.0:
                missed |= (a > 0.0) | (b < 0.0)
                continue
            ta, tb = a / d[k], b / d[k]
            ok = ~(np.isnan(ta) | np.isnan(tb))
            near, far = (ta, tb) if d[k] > 0.0 else (tb, ta)
            tmin = np.where(ok & (near > tmin), near, tmin)
            tmax = np.where(ok & (far < tmax), far, tmax)
        tmin = np.where(np.isfinite(tmin), tmin - SLACK * np.abs(tmin), tmin)
        tmax = np.where(np.isfinite(tmax), tmax + SLACK * np.abs(tmax), tmax)
        return missed | (tmin > tmax) | (tmax < 0.0) | (tmin > best), tmin


def point_skips(p, boxes, slack, best):
    """-> (skip bool [n], bound [n]): bvh_core.h point_skips"""
    with np.errstate(all="ignore"):
        s = []
        for k in range(3):
            below, above = boxes[:, k] - p[k], p[k] - boxes[:, 3 + k]
            e = np.zeros(len(boxes))
            e = np.where(below > e, below, e)
            e = np.where(above > e, above, e)
            s.append(e * e)
        bound = (s[0] + s[1]) + s[2]
        return bound > best + slack, bound


class _Ray:
    def __init__(self, o, d, root):
        self.o, self.d, self.best, self.face = o, d, np.inf, -1
        self.scale = query_scale(o, root)

    def skips(self, boxes):
        return ray_skips(self.o, self.d, boxes, self.scale, self.best)

    def wanted(self, bound):
        return not bound > self.best

    def done(self):
        return False

    def values(self, tri):
        det, un, vn, tn = lo.numerators(self.o[None, None, :], self.d[None, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        with np.errstate(all="ignore"):
            fin = np.isfinite(det) & np.isfinite(un) & np.isfinite(vn) & np.isfinite(tn)
            ins = fin & (((det > 0) & (un >= 0) & (vn >= 0) & (un + vn <= det)) | ((det < 0) & (un <= 0) & (vn <= 0) & (un + vn >= det)))
            t = tn / det
            return np.where(ins & (t > 0.0) & (t < np.inf), t, np.inf)[0]


class _Segment(_Ray):
    """any hit below t_max on a face that does not name `skip`: the bound stays t_max, the walk ends with the first hit"""

    def __init__(self, a, b, root, skip, t_max, faces):
        with np.errstate(all="ignore"):
            super().__init__(a, b - a, root)
        self.t_max, self.skip, self.faces, self.ids = t_max, skip, faces, None

    def skips(self, boxes):
        return ray_skips(self.o, self.d, boxes, self.scale, self.t_max)

    def wanted(self, bound):
        return not bound > self.t_max

    def done(self):
        return self.face >= 0

    def values(self, tri):
        t = super().values(tri)
        named = (self.faces[self.ids] == self.skip).any(1) if self.skip >= 0 else np.zeros(len(t), dtype=bool)
        return np.where((t < self.t_max) & ~named, t, np.inf)


class _Point:
    def __init__(self, p, root):
        self.p, self.best, self.face = p, np.inf, -1
        scale = query_scale(p, root)
        with np.errstate(all="ignore"):
            self.slack = SLACK * (scale * scale)

    def skips(self, boxes):
        return point_skips(self.p, boxes, self.slack, self.best)

    def wanted(self, bound):
        with np.errstate(all="ignore"):
            return not bound > self.best + self.slack

    def done(self):
        return False

    def values(self, tri):
        _, _, d2 = to.closest(self.p[None, :], tri)
        with np.errstate(all="ignore"):
            return np.where(d2[0] < np.inf, d2[0], np.inf)                              # NaN -> +inf: never wins


def _enter(tree, q, level, node, visits):
    """node `node` of level `level` has been entered; level 0: the 64 sorted faces of a level-1 node"""
    first = node * WIDTH
    if level == 0:
        ids = tree["order"][first:first + WIDTH]
        visits[0] += len(ids)
        q.ids = ids
        v = q.values(tree["verts"][tree["faces"][ids]])
        for value, f in zip(v, ids):
            if value < q.best or (value == q.best and value < np.inf and f < q.face):
                q.best, q.face = value, int(f)
        return
    if level == 1:
        _enter(tree, q, 0, node, visits)
        return
    boxes = tree["levels"][level - 2][first:first + WIDTH]
    visits[0] += len(boxes)
    skip, bound = q.skips(boxes)
    pending = sorted((b, c) for c, (s, b) in enumerate(zip(skip, bound)) if not s)      # the smallest bound first, then the lowest child
    for b, c in pending:
        if q.done() or not q.wanted(b):
            break                                                                       # every later bound is at least this one
        _enter(tree, q, level - 1, first + c, visits)


def _walk(tree, q):
    visits = [0]
    top = len(tree["levels"])
    visits[0] += 1                                                                      # the root's own box
    skip, _ = q.skips(tree["levels"][top - 1][:1])
    if not skip[0]:
        _enter(tree, q, top, 0, visits)
    return visits[0]


def cast(tree, origins, dirs, orientation=0):
    """-> dict(t, face, point, visits, bad): the walk of every ray of one mesh"""
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    R = len(o)
    t, face, point, visits = np.full(R, np.inf), np.full(R, -1, dtype=np.int32), np.full((R, 3), np.nan), np.zeros(R, dtype=np.int32)
    for r in range(R if tree["levels"] else 0):
        q = _Ray(o[r], d[r], tree["levels"][-1][0])
        visits[r] = _walk(tree, q)
        if q.face >= 0:
            A, B, C = (tree["verts"][tree["faces"][q.face, k]][None, None, :] for k in range(3))
            det = lo.numerators(o[r][None, None, :], d[r][None, None, :], A, B, C)[0][0, 0]
            if not ((orientation > 0 and not det < 0) or (orientation < 0 and not det > 0)):
                with np.errstate(all="ignore"):
                    t[r], face[r], point[r] = q.best, q.face, o[r] + q.best * d[r]
    return dict(t=t, face=face, point=point, visits=visits, bad=tree["bad"] and R > 0)


def closest(tree, points):
    """-> dict(face, bary, distance, visits, bad, no_faces): the walk of every point of one mesh"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    P = len(p)
    face, bary, dist, visits = np.full(P, -1, dtype=np.int32), np.full((P, 3), np.nan), np.full(P, np.nan), np.zeros(P, dtype=np.int32)
    for i in range(P if tree["levels"] else 0):
        q = _Point(p[i], tree["levels"][-1][0])
        visits[i] = _walk(tree, q)
        if q.face >= 0:
            _, b, _ = to.closest(p[i][None, :], tree["verts"][tree["faces"][q.face]][None])
            face[i], bary[i], dist[i] = q.face, b[0, 0], np.sqrt(q.best)
    return dict(face=face, bary=bary, distance=dist, visits=visits, bad=tree["bad"] and P > 0, no_faces=len(tree["faces"]) == 0 and P > 0)


def _segment_args(a, b, skip_vertex, t_max):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    skip = np.full(len(a), -1, dtype=np.int64) if skip_vertex is None else np.asarray(skip_vertex, dtype=np.int64)
    tm = np.ones(len(a)) if t_max is None else np.asarray(t_max, dtype=np.float64)
    return a, b, skip, tm


def brute_blocked(a, b, verts, faces, skip_vertex=None, t_max=None):
    """-> dict(blocked uint8 [S], bad): the rule of morig_bvh_blocked over all faces of one mesh"""
    a, b, skip, tm = _segment_args(a, b, skip_vertex, t_max)
    fc, bad = clamped(verts, faces)
    out = np.zeros(len(a), dtype=np.uint8)
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    for s in range(len(a) if len(fc) else 0):
        with np.errstate(all="ignore"):
            q = _Segment(a[s], b[s], np.zeros(6), skip[s], tm[s], fc)
        q.ids = np.arange(len(fc))
        out[s] = np.any(q.values(verts[fc]) < np.inf)
    return dict(blocked=out, bad=bad and len(a) > 0)


def blocked(tree, a, b, skip_vertex=None, t_max=None):
    """-> dict(blocked, visits, bad): the walk of every segment of one mesh"""
    a, b, skip, tm = _segment_args(a, b, skip_vertex, t_max)
    out, visits = np.zeros(len(a), dtype=np.uint8), np.zeros(len(a), dtype=np.int32)
    for s in range(len(a) if tree["levels"] else 0):
        q = _Segment(a[s], b[s], tree["levels"][-1][0], skip[s], tm[s], tree["faces"])
        q.best = tm[s]
        visits[s] = _walk(tree, q)
        out[s] = q.face >= 0
    return dict(blocked=out, visits=visits, bad=tree["bad"] and len(a) > 0)


def same(a, b):
    """bit equality, NaN against NaN included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
