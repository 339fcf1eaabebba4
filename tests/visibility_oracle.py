"""NumPy restatement of the two visibility rules on the mesh BVH (csrc/bvh.hip, csrc/bonevis_core.h), for the CPU
tests and as the reference of the GPU tests. It holds

    the view trees     the order of a mesh's faces from ONE pose (tests/spatial_oracle.py build), the boxes from another
    ray_skips          csrc/bvh_core.h ray_skips with the pad's share of the scale as a parameter
    the two queries    on tests/spatial_oracle.py ``_walk``, with the count of box and face tests
    the brute force    both rules over all faces, every operation in the order scan_visibility_kernel (csrc/scan.hip) and
                       bone_visibility_kernel (csrc/geodesic.hip) write it

One view / one mesh at a time; the batch is the callers'."""
import numpy as np

import scan_oracle as sco
import spatial_oracle as so

BONE_SLACK = 2.0 ** -36
ORTHOGRAPHIC, PINHOLE = 0, 1


# ------------------------------------------------------------------------------------------------------------------------- entering
def ray_skips(o, d, boxes, scale, best, slack=so.SLACK):
    """boxes [n, 6] -> (skip bool [n], bound [n]): bvh_core.h ray_skips, the boxes padded by ``slack`` x scale"""
    n = len(boxes)
    with np.errstate(all="ignore"):
        pad = slack * scale
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
        tmin = np.where(np.isfinite(tmin), tmin - so.SLACK * np.abs(tmin), tmin)
        tmax = np.where(np.isfinite(tmax), tmax + so.SLACK * np.abs(tmax), tmax)
        return missed | (tmin > tmax) | (tmax < 0.0) | (tmin > best), tmin


# ------------------------------------------------------------------------------------------------------------------------- view trees
def mesh_order(first_verts, faces):
    """the order of a mesh's faces from the vertices of its first view"""
    return so.build(first_verts, faces)["order"]


def view_tree(verts, faces, order):
    """the tree of a view: the faces in the mesh's order, the boxes exact for the view's own vertices"""
    return so.build(verts, faces, order=order)


# ------------------------------------------------------------------------------------------------------------------------- the scan rule
def scan_rays(verts, cam, kind, W, H):
    """-> (c [V, 3], d [V, 3], len [V], seen bool [V]) as scan_visibility_kernel computes them"""
    verts, cam = np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(cam, dtype=np.float64)
    V = len(verts)
    eye, f, r, u, px, py, near = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12], cam[13], cam[14]
    with np.errstate(all="ignore"):
        de = verts - eye
        z, a, b = sco.dot3(de, f), sco.dot3(de, r), sco.dot3(de, u)
        if kind == PINHOLE:
            a, b = a / z, b / z
            c = np.broadcast_to(eye, (V, 3)).copy()
        else:
            c = verts - z[:, None] * f
        d = verts - c
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        seen = (z > near) & (np.abs(a) <= float(W) * px) & (np.abs(b) <= float(H) * py)
    return c, d, ln, seen


def _blocks(c, d, ln, vis_eps, A, B, C):
    """the face predicate without the corner test: broadcast over rays and faces"""
    det, un, vn, tn = sco.numerators(c, d, A, B, C)
    with np.errstate(all="ignore"):
        t = tn / det
        return sco.inside(det, un, vn, tn) & (t > 0.0) & (t < 1.0) & (t * ln < ln - vis_eps), t


def brute_scan(verts, faces, cam, kind, W, H, vis_eps):
    """-> dict(vis uint8 [V], seen, bad): morig_scan_visibility on one view, over all faces"""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    fc, bad = so.clamped(verts, faces)
    c, d, ln, seen = scan_rays(verts, cam, kind, W, H)
    blocked, ids = np.zeros(len(verts), dtype=bool), np.arange(len(verts))
    for fa, fb, fcn in fc:
        hit, _ = _blocks(c, d, ln, vis_eps, verts[fa], verts[fb], verts[fcn])
        blocked |= hit & (ids != fa) & (ids != fb) & (ids != fcn)
    return dict(vis=(seen & ~blocked).astype(np.uint8), seen=seen, bad=bad and len(verts) > 0)


class _Scan:
    """any face that blocks the vertex: the bound stays 1, the walk ends with the first leaf that holds one"""

    def __init__(self, c, d, ln, vis_eps, me, root, faces):
        self.o, self.d, self.ln, self.vis_eps, self.me, self.faces = c, d, ln, vis_eps, me, faces
        self.best, self.face, self.ids = 1.0, -1, None
        self.scale = so.query_scale(c, root)

    def skips(self, boxes):
        return ray_skips(self.o, self.d, boxes, self.scale, 1.0)

    def wanted(self, bound):
        return not bound > 1.0

    def done(self):
        return self.face >= 0

    def values(self, tri):
        hit, t = _blocks(self.o[None, :], self.d[None, :], self.ln, self.vis_eps, tri[:, 0], tri[:, 1], tri[:, 2])
        named = (self.faces[self.ids] == self.me).any(1)
        return np.where(hit & ~named, t, np.inf)


def walk_scan(tree, cam, kind, W, H, vis_eps):
    """-> dict(vis, visits int32 [V], bad): the walk of every vertex of one view over its view tree"""
    verts = tree["verts"]
    c, d, ln, seen = scan_rays(verts, cam, kind, W, H)
    vis, visits = seen.copy(), np.zeros(len(verts), dtype=np.int32)
    for v in range(len(verts) if tree["levels"] else 0):
        if not seen[v]:
            continue                                                                    # outside the frustum: nothing is walked
        with np.errstate(all="ignore"):
            q = _Scan(c[v], d[v], ln[v], vis_eps, v, tree["levels"][-1][0], tree["faces"])
        visits[v] = so._walk(tree, q)
        vis[v] = q.face < 0
    return dict(vis=vis.astype(np.uint8), visits=visits, bad=tree["bad"] and len(verts) > 0)


# ------------------------------------------------------------------------------------------------------------------------- the bone rule
def bone_rays(pos, bones):
    """every (vertex, bone) pair, vertex-major as the kernels lay them out -> (o [P, 3], d [P, 3], len [P], dn [P]): bonevis_core.h
    ray_of, with pt2line's zero-length-bone branch"""
    pos, bones = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(bones, dtype=np.float64).reshape(-1, 6)
    V, nb = len(pos), len(bones)
    p = np.repeat(pos, nb, axis=0)
    bn = np.tile(bones, (V, 1))
    with np.errstate(all="ignore"):
        a, e = bn[:, 0:3], bn[:, 3:6] - bn[:, 0:3]
        l2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        t = (((p[:, 0] - a[:, 0]) * e[:, 0] + (p[:, 1] - a[:, 1]) * e[:, 1]) + (p[:, 2] - a[:, 2]) * e[:, 2]) / l2
        t = np.fmin(np.fmax(t, 0.0), 1.0)                                               # fmin / fmax: a NaN gives the other operand
        o = np.where((np.abs(l2) < 1e-8)[:, None], a, a + t[:, None] * e)
        r = p - o
        ln = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        d = r + 1e-15
        dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return o, d, ln, dn


def bone_hits(o, d, dn, A, B, C):
    """one ray against the faces (A, B, C) [n, 3] -> t [n], +inf where the tolerance Moeller-Trumbore of bonevis_core.h misses"""
    with np.errstate(all="ignore"):
        dx, dy, dz = d
        e1x, e1y, e1z = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1], B[:, 2] - A[:, 2]
        e2x, e2y, e2z = C[:, 0] - A[:, 0], C[:, 1] - A[:, 1], C[:, 2] - A[:, 2]
        nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
        area = np.sqrt((nx * nx + ny * ny) + nz * nz)
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = (e1x * px + e1y * py) + e1z * pz
        ok = np.abs(det) > 1e-12 * dn * area
        inv = 1.0 / det
        tx, ty, tz = o[0] - A[:, 0], o[1] - A[:, 1], o[2] - A[:, 2]
        u = ((tx * px + ty * py) + tz * pz) * inv
        ok &= ~((u < -1e-12) | (u > 1.0 + 1e-12))
        qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
        v = ((dx * qx + dy * qy) + dz * qz) * inv
        ok &= ~((v < -1e-12) | (u + v > 1.0 + 1e-12))
        t = ((e2x * qx + e2y * qy) + e2z * qz) * inv
        return np.where(ok & (t > 0.0), t, np.inf)


def hit_distance(d, t):
    with np.errstate(all="ignore"):
        hx, hy, hz = t * d[0], t * d[1], t * d[2]
        return np.sqrt((hx * hx + hy * hy) + hz * hz)


def visible(min_hit, ln):
    with np.errstate(all="ignore"):
        return bool(np.abs((ln if np.isinf(min_hit) else min_hit) - ln) < 1e-4)


def decides(h, ln):
    with np.errstate(all="ignore"):
        return bool(h < ln and not np.abs(h - ln) < 1e-4)


def brute_bone(pos, bones, tri_pos, faces):
    """-> dict(vis uint8 [V * nb], min_hit [V * nb], bad): morig_bone_visibility on one mesh, the minimum over h as the kernel takes it"""
    tri_pos = np.asarray(tri_pos, dtype=np.float64).reshape(-1, 3)
    fc, bad = so.clamped(tri_pos, faces)
    o, d, ln, dn = bone_rays(pos, bones)
    vis, low = np.zeros(len(o), dtype=np.uint8), np.full(len(o), np.inf)
    A, B, C = (tri_pos[fc[:, k]] for k in range(3)) if len(fc) else (np.zeros((0, 3)),) * 3
    for i in range(len(o)):
        t = bone_hits(o[i], d[i], dn[i], A, B, C)
        with np.errstate(all="ignore"):
            h = hit_distance(d[i][:, None], t)                                          # h per face; a NaN (inf x 0) is never below the minimum
        h = h[(t < np.inf) & ~np.isnan(h)]
        low[i] = h.min() if len(h) else np.inf
        vis[i] = visible(low[i], ln[i])
    return dict(vis=vis, min_hit=low, bad=bad and len(o) > 0)


class _Bone:
    """the nearest hit on t, boxes padded by BONE_SLACK of the scale; ended by a hit that decides"""

    def __init__(self, o, d, ln, dn, root):
        self.o, self.d, self.ln, self.dn = o, d, ln, dn
        self.best, self.face, self.ids = np.inf, -1, None
        self.scale = so.query_scale(o, root)

    def skips(self, boxes):
        return ray_skips(self.o, self.d, boxes, self.scale, self.best, BONE_SLACK)

    def wanted(self, bound):
        return not bound > self.best

    def done(self):
        return self.face >= 0 and decides(hit_distance(self.d, self.best), self.ln)

    def values(self, tri):
        return bone_hits(self.o, self.d, self.dn, tri[:, 0], tri[:, 1], tri[:, 2])


def walk_bone(tree, pos, bones):
    """-> dict(vis, visits int32 [V * nb], bad): the walk of every (vertex, bone) pair of one mesh over its occluder's tree"""
    o, d, ln, dn = bone_rays(pos, bones)
    vis, visits = np.zeros(len(o), dtype=np.uint8), np.zeros(len(o), dtype=np.int32)
    for i in range(len(o)):
        h = np.inf
        if tree["levels"]:
            with np.errstate(all="ignore"):
                q = _Bone(o[i], d[i], ln[i], dn[i], tree["levels"][-1][0])
            visits[i] = so._walk(tree, q)
            if q.face >= 0:
                h = hit_distance(d[i], q.best)
        vis[i] = visible(h, ln[i])
    return dict(vis=vis, visits=visits, bad=tree["bad"] and len(o) > 0)


def entered_above(tree, position, skips):
    """whether the box of the sorted face at ``position`` and every box above it is entered under ``skips(boxes) -> (skip, bound)``"""
    at = position
    for lv in tree["levels"]:
        at //= so.WIDTH
        if skips(lv[at:at + 1])[0][0]:
            return False
    return True
