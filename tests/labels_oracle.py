"""NumPy restatement of the rule of morig_amd/labels.py and csrc/labels.hip, for the CPU tests and as the reference of
the GPU tests: the bone rays by a loop over the joints, the nearest hit by brute force over all rays x all faces with the numerators of
csrc/raytri_core.h in the same order, the percentile through a sort, the label through a distance matrix. Every stage also reports how
far its decisions were from flipping (the margins), so that a test can leave out what rounding may decide either way. The scenes of the
GPU tests are built here, so that tests/test_labels_oracle.py can bound the left-out share on the CPU."""
import functools
import math

import numpy as np

MARGIN = 1e-9                    # inside / outside, the gap to the second-nearest t, |t - keep_factor p20|
RADIUS_MARGIN = 1e-12            # |dist - radius|


# ------------------------------------------------------------------------------------------------------------------------- rule (1)
def _unit(v):
    return v / math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _length(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def bone_rays(pos, hier, n_rays):
    """one rig, joint after joint -> origins [R, 3], dirs [R, 3], ray_joint [R], rays per joint [J]"""
    pos, hier = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(hier).reshape(-1)
    ang = (2.0 * np.pi * np.arange(n_rays, dtype=np.float64)) / n_rays
    cs, sn = np.cos(ang), np.sin(ang)                                                   # the same numpy call as the product: the same bits
    origins, dirs, ray_joint, counts = [], [], [], []
    for j in range(len(pos)):
        axes = []
        for c in range(len(pos)):
            if hier[c] == j and _length(pos[c] - pos[j]) > 1e-8:
                axes.append((pos[c] - pos[j]) / _length(pos[c] - pos[j]))
        if not axes and hier[j] >= 0 and _length(pos[j] - pos[hier[j]]) > 1e-8:
            axes.append((pos[j] - pos[hier[j]]) / _length(pos[j] - pos[hier[j]]))
        for a in axes:
            e = np.zeros(3)
            e[int(np.argmin(np.abs(a)))] = 1.0
            u = _unit(_cross(a, e))
            w = _cross(a, u)
            for i in range(n_rays):
                origins.append(pos[j])
                dirs.append(cs[i] * u + sn[i] * w)
                ray_joint.append(j)
        counts.append(len(axes) * n_rays)
    return (np.array(origins, dtype=np.float64).reshape(-1, 3), np.array(dirs, dtype=np.float64).reshape(-1, 3),
            np.array(ray_joint, dtype=np.int64), np.array(counts, dtype=np.int64))


# ------------------------------------------------------------------------------------------------------------------------- rule (2)
def numerators(o, d, A, B, C):
    """o, d [R, 1, 3]; A, B, C [1, F, 3] -> det, un, vn, tn [R, F], every operation as raytri_core.h writes it"""
    with np.errstate(all="ignore"):
        e1x, e1y, e1z = B[..., 0] - A[..., 0], B[..., 1] - A[..., 1], B[..., 2] - A[..., 2]
        e2x, e2y, e2z = C[..., 0] - A[..., 0], C[..., 1] - A[..., 1], C[..., 2] - A[..., 2]
        d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
        px, py, pz = d1 * e2z - d2 * e2y, d2 * e2x - d0 * e2z, d0 * e2y - d1 * e2x
        sx, sy, sz = o[..., 0] - A[..., 0], o[..., 1] - A[..., 1], o[..., 2] - A[..., 2]
        qx, qy, qz = sy * e1z - sz * e1y, sz * e1x - sx * e1z, sx * e1y - sy * e1x
        det = (e1x * px + e1y * py) + e1z * pz
        un = (sx * px + sy * py) + sz * pz
        vn = (d0 * qx + d1 * qy) + d2 * qz
        tn = (e2x * qx + e2y * qy) + e2z * qz
    return det, un, vn, tn


def cast(origins, dirs, verts, faces, orientation=0, chunk=32):
    """-> dict(t [R] (+inf), face int32 [R] (-1), point [R, 3] (NaN), margin [R]). margin: the smallest of |inside margin| relative to
    |det| over all faces, t of every inside face relative to 1 (how far a hit is from lying behind the origin), and the relative gap
    between the nearest and the second-nearest t; +inf where no face comes near. Orientation only discards the winner."""
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    verts, faces = np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    R, F = len(o), len(faces)
    assert F == 0 or (faces.min() >= 0 and faces.max() < len(verts))
    t_out, f_out, margin = np.full(R, np.inf), np.full(R, -1, dtype=np.int32), np.full(R, np.inf)
    p_out = np.full((R, 3), np.nan)
    if F == 0 or R == 0:
        return dict(t=t_out, face=f_out, point=p_out, margin=margin)
    A, B, C = verts[faces[:, 0]][None], verts[faces[:, 1]][None], verts[faces[:, 2]][None]
    for r0 in range(0, R, chunk):
        rs = slice(r0, min(r0 + chunk, R))
        det, un, vn, tn = numerators(o[rs, None, :], d[rs, None, :], A, B, C)
        with np.errstate(all="ignore"):
            fin = np.isfinite(det) & np.isfinite(un) & np.isfinite(vn) & np.isfinite(tn)
            ins = fin & (((det > 0) & (un >= 0) & (vn >= 0) & (un + vn <= det)) | ((det < 0) & (un <= 0) & (vn <= 0) & (un + vn >= det)))
            t = tn / det
            hit = ins & (t > 0.0)
            sg = np.sign(det)
            im = np.minimum(np.minimum(sg * un, sg * vn), sg * ((det - un) - vn)) / np.abs(det)
            im = np.abs(np.where(np.isfinite(im), im, -np.inf))
            im = np.where(ins, np.minimum(im, np.abs(t)), im)
        th = np.where(hit, t, np.inf)
        best = np.argmin(th, 1)                                                         # the first minimum: the lowest face among equals
        rows = np.arange(th.shape[0])
        tb = th[rows, best]
        got = tb < np.inf
        second = th.copy()
        second[rows, best] = np.inf
        t2 = second.min(1)
        with np.errstate(all="ignore"):
            gap = np.where(got & (t2 < np.inf), (t2 - tb) / np.abs(tb), np.inf)
        m = np.minimum(im.min(1), np.where(np.isnan(gap), 0.0, gap))
        db = det[rows, best]
        if orientation > 0:
            got = got & (db < 0)
        elif orientation < 0:
            got = got & (db > 0)
        t_out[rs] = np.where(got, tb, np.inf)
        f_out[rs] = np.where(got, best, -1)
        with np.errstate(all="ignore"):
            p_out[rs] = np.where(got[:, None], o[rs] + tb[:, None] * d[rs], np.nan)
        margin[rs] = m
    return dict(t=t_out, face=f_out, point=p_out, margin=margin)


# ------------------------------------------------------------------------------------------------------------------------- rule (3)
def p20_of(hits_sorted):
    n = len(hits_sorted)
    h = 0.2 * (n - 1)
    lo = int(math.floor(h))
    return hits_sorted[lo] + (h - lo) * (hits_sorted[min(lo + 1, n - 1)] - hits_sorted[lo])


def select(t, counts, keep_factor=2.0, fill=float("nan")):
    """t [R], counts [J] -> dict(kept uint8 [R], n_hit, n_kept int32 [J], p20, featuresize [J], margin [R] = |t - keep_factor p20| of the
    hits, +inf for a miss)"""
    t, counts = np.asarray(t, dtype=np.float64).reshape(-1), np.asarray(counts, dtype=np.int64).reshape(-1)
    J = len(counts)
    kept, margin = np.zeros(len(t), dtype=np.uint8), np.full(len(t), np.inf)
    n_hit, n_kept = np.zeros(J, dtype=np.int32), np.zeros(J, dtype=np.int32)
    p20, fs = np.full(J, np.nan), np.full(J, float(fill))
    at = 0
    for j in range(J):
        tj = t[at:at + counts[j]]
        hit = tj < np.inf
        n_hit[j] = hit.sum()
        if n_hit[j]:
            p20[j] = p20_of(np.sort(tj[hit]))
            thr = keep_factor * p20[j]
            with np.errstate(all="ignore"):
                k = hit & (tj <= thr)
                margin[at:at + counts[j]] = np.where(hit, np.abs(tj - thr), np.inf)
            kept[at:at + counts[j]] = k
            n_kept[j] = k.sum()
            if n_kept[j]:
                s = 0.0
                for x in tj[k]:                                                         # ascending ray order
                    s = s + float(x)
                fs[j] = s / float(n_kept[j])
        at += counts[j]
    return dict(kept=kept, n_hit=n_hit, n_kept=n_kept, p20=p20, featuresize=fs, margin=margin)


# ------------------------------------------------------------------------------------------------------------------------- rule (4)
def attention(verts, point, kept, radius=0.02):
    """-> (attn float32 [V], margin [V]: the smallest |dist - radius| over the kept hits, +inf without one)"""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    pts = np.asarray(point, dtype=np.float64).reshape(-1, 3)[np.asarray(kept).reshape(-1) != 0]
    if len(pts) == 0 or len(verts) == 0:
        return np.zeros(len(verts), dtype=np.float32), np.full(len(verts), np.inf)
    dx, dy, dz = (verts[:, None, k] - pts[None, :, k] for k in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    attn = (d2 <= radius * radius).any(1).astype(np.float32)
    return attn, np.abs(np.sqrt(d2) - radius).min(1)


def labels(verts, faces, pos, hier, n_rays=14, keep_factor=2.0, radius=0.02, orientation=0, fill=float("nan")):
    """one mesh -> dict: attn, featuresize, t, face, point, kept, ray_joint, n_hit, n_kept, p20 and the margins ray_margin [R] (cast),
    keep_margin [R], radius_margin [V]"""
    o, d, ray_joint, counts = bone_rays(pos, hier, n_rays)
    c = cast(o, d, verts, faces, orientation)
    s = select(c["t"], counts, keep_factor, fill)
    attn, rm = attention(verts, c["point"], s["kept"], radius)
    return dict(attn=attn, featuresize=s["featuresize"], t=c["t"], face=c["face"], point=c["point"], kept=s["kept"], ray_joint=ray_joint,
                n_hit=s["n_hit"], n_kept=s["n_kept"], p20=s["p20"], ray_margin=c["margin"], keep_margin=s["margin"], radius_margin=rm,
                origins=o, dirs=d, counts=counts)


# ------------------------------------------------------------------------------------------------------------------------- scenes
class PlainRig:
    """what the product reads of a rig: pos, hierarchy, names, skins"""

    def __init__(self, pos, hier):
        self.pos, self.hierarchy = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(hier, dtype=np.int64).reshape(-1)
        self.names = [f"joint_{i}" for i in range(len(self.pos))]
        self.skins = []


def torus_mesh(n_side, R=0.35, r=0.12, noise=1e-3, seed=0):
    """an n_side x n_side triangulated torus about the y axis with its core circle in the plane y = 0, vertex noise of `noise`"""
    rng = np.random.default_rng([0x4C61626C, seed, n_side])
    a = (np.arange(n_side) / n_side) * 2.0 * np.pi
    uu, vv = np.meshgrid(a, a, indexing="ij")
    v = np.stack([(R + r * np.cos(vv)) * np.cos(uu), r * np.sin(vv), (R + r * np.cos(vv)) * np.sin(uu)], -1).reshape(-1, 3)
    v = v + rng.normal(0.0, noise, size=v.shape)
    idx = np.arange(n_side * n_side).reshape(n_side, n_side)
    i00, i10, i01, i11 = idx, np.roll(idx, -1, 0), np.roll(idx, -1, 1), np.roll(np.roll(idx, -1, 0), -1, 1)
    f = np.concatenate([np.stack([i00, i10, i11], -1).reshape(-1, 3), np.stack([i00, i11, i01], -1).reshape(-1, 3)], 0)
    return v, f.astype(np.int64)


def torus_chain(n_joints=12, R=0.35, jitter=0.01, seed=0):
    """a chain of joints on the core circle, jittered off the symmetry positions so that no ray runs through a mesh vertex"""
    rng = np.random.default_rng([0x4A6F696E, seed, n_joints])
    ang = 2.0 * np.pi * (np.arange(n_joints) + rng.uniform(0.1, 0.4, n_joints)) / (n_joints + 1)
    pos = np.stack([R * np.cos(ang), np.zeros(n_joints), R * np.sin(ang)], 1) + rng.uniform(-jitter, jitter, size=(n_joints, 3))
    return pos, np.arange(-1, n_joints - 1, dtype=np.int64)


GENERATED_SIDES = (16, 32, 64)


@functools.lru_cache(maxsize=None)
def generated_scene(n_side, seed=0):
    v, f = torus_mesh(n_side, seed=seed)
    pos, hier = torus_chain(seed=seed)
    return v, f, pos, hier


@functools.lru_cache(maxsize=None)
def generated_reference(n_side, seed=0):
    v, f, pos, hier = generated_scene(n_side, seed)
    return labels(v, f, pos, hier)


def box_mesh(hx, hy, hz):
    s = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-hz, hz)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return s, np.array(f, dtype=np.int64)


# on a coarse binary grid every product of the ray test is exact: the device must give the oracle's bits with nothing excused
def on_grid_scene():
    """-> (verts, faces, origins, dirs, names): one mesh, one ray per named case, axis-aligned directions"""
    nan = np.nan
    verts = np.array([[0, 0, 2], [1, 0, 2], [1, 1, 2], [0, 1, 2],                       # 0-3   a square at z = 2, normals +z
                      [4, 0, 3], [5, 0, 3], [5, 1, 3], [4, 0, 2], [5, 0, 2], [5, 1, 2],  # 4-9   plates at x = 4..5: z = 3 (normal -z), z = 2 (+z)
                      [0, 4, 1], [0.5, 4.5, 1], [1, 5, 1], [0, 4, 2], [2, 4, 2], [0, 6, 2],   # 10-15 a zero-area face in front of a plate
                      [4, 4, 1], [5, 4, nan], [4, 5, 1], [4, 4, 2], [6, 4, 2], [4, 6, 2],     # 16-21 a face with a NaN vertex in front of a plate
                      [8, 0, 2], [9, 0, 2], [8, 1, 2], [8, 0, 2], [9, 0, 2], [8, 1, 2]],      # 22-27 the same triangle twice
                     dtype=np.float64)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [7, 8, 9], [10, 11, 12], [13, 14, 15], [16, 17, 18], [19, 20, 21], [25, 26, 27], [22, 23, 24]])
    rays = {"inside": ([0.75, 0.25, 0], [0, 0, 1]), "shared_edge": ([0.5, 0.5, 0], [0, 0, 1]), "corner": ([0, 0, 0], [0, 0, 1]),
            "far_corner": ([1, 1, 0.5], [0, 0, 2]), "outer_edge": ([1, 0.5, 0], [0, 0, 1]), "outside": ([1.25, 0.5, 0], [0, 0, 1]),
            "coplanar": ([-1, 0.25, 2], [1, 0, 0]), "behind": ([0.75, 0.25, 3], [0, 0, 1]), "from_above": ([0.75, 0.25, 3], [0, 0, -1]),
            "on_the_face": ([0.75, 0.25, 2], [0, 0, 1]), "two_plates": ([4.75, 0.25, 0], [0, 0, 1]), "two_plates_down": ([4.75, 0.25, 4], [0, 0, -0.5]),
            "zero_area": ([0.25, 4.25, 0], [0, 0, 1]), "nan_vertex": ([4.25, 4.25, 0], [0, 0, 1]), "twins": ([8.25, 0.25, 0], [0, 0, 1]),
            "nan_ray": ([0.75, nan, 0], [0, 0, 1]), "zero_dir": ([0.75, 0.25, 0], [0, 0, 0]), "sideways": ([-2, 0.5, 2.5], [1, 0, 0])}
    names = list(rays)
    return (verts, faces, np.array([rays[n][0] for n in names], dtype=np.float64), np.array([rays[n][1] for n in names], dtype=np.float64), names)


def grid_triangles(n_faces, seed):
    """n_faces triangles with corners on the grid of eighths in [0, 4]^3 (exact products), some of them degenerate"""
    rng = np.random.default_rng([0x47726964, seed, n_faces])
    v = rng.integers(0, 33, size=(max(3 * n_faces, 1), 3)).astype(np.float64) / 8.0
    return v, np.arange(3 * n_faces, dtype=np.int64).reshape(n_faces, 3)


def grid_rays(n, seed):
    """n axis-aligned rays from grid points of [0, 4]^3, signs and axes mixed"""
    rng = np.random.default_rng([0x52617973, seed, n])
    o = rng.integers(0, 33, size=(n, 3)).astype(np.float64) / 8.0
    d = np.zeros((n, 3))
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0, 0.5], n)
    return o, d


def hit_set(n, seed):
    """n hit distances with ties and misses, as a joint may have them"""
    rng = np.random.default_rng([0x48697473, seed, n])
    t = rng.uniform(0.05, 0.3, n)
    if n >= 5:
        t[rng.integers(0, n, n // 5)] = t[0]                                            # ties
        t[rng.integers(0, n, n // 4)] = np.inf                                          # misses
        t[rng.integers(0, n, 1)] = 5.0                                                  # one far hit that is not kept
    return t
