"""NumPy restatement of the rules of morig_amd/scan.py and csrc/scan.hip, for the CPU tests and as the reference of
the GPU tests: brute force over all pixels x all faces with the numerators of csrc/raytri_core.h in the same order, the key rule, the
segment rule of the visibility mask and the nearest search with lowest-index ties. Every function also reports how far a decision was
from flipping (its margin), so that a test can leave out what rounding may decide either way. The scenes of the GPU tests are built
here, so that tests/test_scan_oracle.py can bound the left-out share on the CPU."""
import functools

import numpy as np

import point_oracle

MARGIN = 1e-9
NO_HIT = np.uint64(0xFFFFFFFFFFFFFFFF)
ORTHOGRAPHIC, PINHOLE = 0, 1


# ------------------------------------------------------------------------------------------------------------------------- rays, triangles
def pixel_rays(cam, kind, W, H):
    """cam: the 16 doubles (eye, f, r, u, px, py, near, 0) -> origins [H, W, 3], directions [H, W, 3]"""
    cam = np.asarray(cam, dtype=np.float64)
    eye, f, r, u, px, py = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12], cam[13]
    a = (((2 * np.arange(W) + 1) - W).astype(np.float64) * px)[None, :, None]
    b = ((H - (2 * np.arange(H) + 1)).astype(np.float64) * py)[:, None, None]
    if kind == PINHOLE:
        return np.broadcast_to(eye, (H, W, 3)).copy(), (f + a * r) + b * u
    return (eye + a * r) + b * u, np.broadcast_to(f, (H, W, 3)).copy()


def numerators(o, d, A, B, C):
    """o, d [..., 3]; A, B, C [..., 3] (broadcast) -> det, un, vn, tn, every operation as raytri_core.h writes it"""
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


def inside(det, un, vn, tn):
    with np.errstate(all="ignore"):
        fin = np.isfinite(det) & np.isfinite(un) & np.isfinite(vn) & np.isfinite(tn)
        pos = (det > 0) & (un >= 0) & (vn >= 0) & (un + vn <= det)
        neg = (det < 0) & (un <= 0) & (vn <= 0) & (un + vn >= det)
    return fin & (pos | neg)


def inside_margin(det, un, vn):
    """the signed distance of the inside test from flipping, relative to |det|: >= 0 inside; -inf where det is 0 or no number"""
    with np.errstate(all="ignore"):
        s = np.sign(det)
        m = np.minimum(np.minimum(s * un, s * vn), s * ((det - un) - vn)) / np.abs(det)
    return np.where(np.isfinite(m), m, -np.inf)


def key_of(t, face):
    bits = np.asarray(t, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | np.uint64(face)


# ------------------------------------------------------------------------------------------------------------------------- render
def render(verts, faces, cam, kind, W, H):
    """-> dict(depth [H, W] (+inf), face int32 [H, W] (-1), point [H, W, 3] (+inf), margin [H, W]: the smallest of the inside margins of
    all faces, the distance of a hit's t from near, and the relative gap between the two best keys' depths; inf where no face is near)"""
    verts, faces, cam = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64).reshape(-1, 3), np.asarray(cam, dtype=np.float64)
    o, d = pixel_rays(cam, kind, W, H)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    P, near = W * H, cam[14]
    best, second = np.full(P, NO_HIT), np.full(P, NO_HIT)
    margin = np.full(P, np.inf)
    for fi, (a, b, c) in enumerate(faces):
        A, B, C = verts[a], verts[b], verts[c]
        if not (np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(C).all()):
            continue
        det, un, vn, tn = numerators(o, d, A, B, C)
        with np.errstate(all="ignore"):
            t = tn / det
            ins = inside(det, un, vn, tn)
            hit = ins & (t > near)
            key = np.where(hit, key_of(np.where(hit, t, 1.0), fi), NO_HIT)
            m = np.abs(inside_margin(det, un, vn))
            m = np.where(ins, np.minimum(m, np.abs(t - near)), m)
        margin = np.minimum(margin, m)
        second = np.minimum(second, np.maximum(best, key))
        best = np.minimum(best, key)
    got = best != NO_HIT
    face = np.where(got, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    depth, point = np.full(P, np.inf), np.full((P, 3), np.inf)
    if got.any():
        idx = np.nonzero(got)[0]
        tri = faces[face[idx]]
        det, un, vn, tn = numerators(o[idx], d[idx], verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]])
        t = tn / det
        depth[idx] = t
        point[idx] = o[idx] + t[:, None] * d[idx]
        both = got & (second != NO_HIT)
        t1 = (best >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
        t2 = (second >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            gap = np.where(both, (t2 - t1) / np.abs(t1), np.inf)
        margin = np.minimum(margin, np.where(np.isnan(gap), 0.0, gap))
    return dict(depth=depth.reshape(H, W), face=face.astype(np.int32).reshape(H, W), point=point.reshape(H, W, 3), margin=margin.reshape(H, W))


# ------------------------------------------------------------------------------------------------------------------------- visibility
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def visibility(verts, faces, cam, kind, W, H, vis_eps):
    """-> (vis uint8 [V], firm bool [V]): firm where no part of the decision was within MARGIN of flipping"""
    verts, faces, cam = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64).reshape(-1, 3), np.asarray(cam, dtype=np.float64)
    V = len(verts)
    eye, f, r, u, px, py, near = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12], cam[13], cam[14]
    with np.errstate(all="ignore"):
        de = verts - eye
        z, a, b = dot3(de, f), dot3(de, r), dot3(de, u)
        if kind == PINHOLE:
            a, b = a / z, b / z
            c = np.broadcast_to(eye, (V, 3))
        else:
            c = verts - z[:, None] * f
        d = verts - c
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        seen = (z > near) & (np.abs(a) <= W * px) & (np.abs(b) <= H * py)
        frame_margin = np.minimum(np.minimum(W * px - np.abs(a), H * py - np.abs(b)), z - near)
        frame_margin = np.where(np.isfinite(frame_margin), frame_margin, -np.inf)
    blocked, firm_block, all_firm_miss = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool), np.ones(V, dtype=bool)
    ids = np.arange(V)
    for fa, fb, fc in faces:
        A, B, C = verts[fa], verts[fb], verts[fc]
        det, un, vn, tn = numerators(c, d, A, B, C)
        other = (ids != fa) & (ids != fb) & (ids != fc)
        with np.errstate(all="ignore"):
            t = tn / det
            blocks = other & inside(det, un, vn, tn) & (t > 0) & (t < 1) & (t * ln < ln - vis_eps)
            bm = np.minimum(np.minimum(inside_margin(det, un, vn), np.minimum(t, 1 - t)), (ln - vis_eps) - t * ln)
            bm = np.where(np.isnan(bm), -np.inf, bm)
        blocked |= blocks
        firm_block |= other & blocks & (bm > MARGIN)
        all_firm_miss &= ~other | (~blocks & (bm < -MARGIN))
    vis = seen & ~blocked
    firm = (frame_margin < -MARGIN) | ((frame_margin > MARGIN) & (firm_block | all_firm_miss))
    return vis.astype(np.uint8), firm


# ------------------------------------------------------------------------------------------------------------------------- nearest, scan
def nearest(q, t, mask=None):
    """-> (idx int32 [Q], the lowest index among the nearest shown targets or -1; d2 float64 [Q], +inf without one)"""
    q, t = np.asarray(q, dtype=np.float64).reshape(-1, 3), np.asarray(t, dtype=np.float64).reshape(-1, 3)
    idx, d2 = np.full(len(q), -1, dtype=np.int32), np.full(len(q), np.inf)
    shown = np.ones(len(t), dtype=bool) if mask is None else np.asarray(mask) != 0
    if len(t) == 0 or len(q) == 0:
        return idx, d2
    with np.errstate(all="ignore"):
        dx, dy, dz = q[:, None, 0] - t[None, :, 0], q[:, None, 1] - t[None, :, 1], q[:, None, 2] - t[None, :, 2]
        dd = (dx * dx + dy * dy) + dz * dz
    dd = np.where(shown[None, :] & ~np.isnan(dd), dd, np.inf)
    arg = np.argmin(dd, axis=1)                                                      # the first minimum
    low = dd[np.arange(len(q)), arg]
    ok = low < np.inf
    idx[ok], d2[ok] = arg[ok], low[ok]
    return idx, d2


def fps32(pts, n):
    """morig_fps on one cloud: float32 positions, started at point 0, the first maximum -> local indices"""
    p4 = np.zeros((len(pts), 4), dtype=np.float32)
    p4[:, :3] = np.asarray(pts, dtype=np.float64).astype(np.float32)
    return point_oracle.fps(p4, np.array([0, len(pts)]), np.array([0, n])).astype(np.int64)


def scan_from_images(verts, face_img, point_img, vis, n_pts=None, corr_radius=0.02):
    """what scan_meshes makes of a view's images and visibility mask -> dict(pts, pixel, face, corr_v2p, corr_p2v)"""
    face = np.asarray(face_img).reshape(-1)
    pixel = np.nonzero(face >= 0)[0]
    pts, hit_face = np.asarray(point_img).reshape(-1, 3)[pixel], face[pixel].astype(np.int64)
    if n_pts is not None:
        keep = fps32(pts, n_pts)
        pts, pixel, hit_face = pts[keep], pixel[keep], hit_face[keep]
    r2, vis = corr_radius * corr_radius, np.asarray(vis) != 0
    vi, vd = nearest(verts, pts)
    rows = np.nonzero(vis & (vi >= 0) & (vd <= r2))[0]
    v2p = np.stack([rows, vi[rows].astype(np.int64)], 1).astype(np.int64).reshape(-1, 2)
    pi, pd = nearest(pts, verts, vis)
    rows = np.nonzero((pi >= 0) & (pd <= r2))[0]
    p2v = np.stack([rows, pi[rows].astype(np.int64)], 1).astype(np.int64).reshape(-1, 2)
    return dict(pts=pts, pixel=pixel.astype(np.int64), face=hit_face, corr_v2p=v2p, corr_p2v=p2v)


# ------------------------------------------------------------------------------------------------------------------------- scenes
def sphere(n_lon=32, n_lat=16, radius=1.0):
    """a UV sphere of n_lon x n_lat faces (quads as two triangles, fans at the poles are degenerate-free): vertices on the sphere"""
    verts = [[0.0, radius, 0.0]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            verts.append([radius * np.sin(th) * np.cos(ph), radius * np.cos(th), radius * np.sin(th) * np.sin(ph)])
    verts.append([0.0, -radius, 0.0])
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    faces = []
    for j in range(n_lon):
        faces.append([0, ring(1, j + 1), ring(1, j)])
        faces.append([len(verts) - 1, ring(n_lat - 1, j), ring(n_lat - 1, j + 1)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            faces.append([ring(i, j), ring(i, j + 1), ring(i + 1, j)])
            faces.append([ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j)])
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


def rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def torus(n=24, R=0.6, r=0.25, seed=5):
    """a closed n x n torus, rotated by a fixed random rotation (no face is aligned with a pixel row)"""
    a = 2 * np.pi * np.arange(n) / n
    u, v = np.meshgrid(a, a, indexing="ij")
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3) @ rotation(seed).T
    at = lambda i, j: (i % n) * n + j % n
    faces = [[[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]] for i in range(n) for j in range(n)]
    return np.ascontiguousarray(verts), np.array(faces, dtype=np.int64).reshape(-1, 3)


def random_triangles(n=200, seed=9):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.8, 0.8, size=(n, 1, 3))
    verts = (centre + rng.normal(scale=0.15, size=(n, 3, 3))).reshape(-1, 3)
    return verts, np.arange(3 * n, dtype=np.int64).reshape(-1, 3)


def generated_cameras(W, H):
    """the two cameras of the generated scenes, as the arguments of morig_amd.scan.Camera.orthographic / .pinhole (the tests build them
    with the product's Camera; this module imports nothing of the package)"""
    return {"orthographic": dict(eye=(0.3, 0.4, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), half_width=1.1, half_height=1.1 * H / W,
                                 width=W, height=H),
            "pinhole": dict(eye=(0.5, 0.7, 2.6), target=(0.0, 0.05, 0.0), up=(0.1, 1.0, 0.0), fov_y_deg=42.0, width=W, height=H)}


GEN_W, GEN_H = 96, 80


def generated_scenes():
    return {"torus": torus(), "triangles": random_triangles()}


@functools.lru_cache(maxsize=None)
def generated_reference(scene, cam_row, kind, W=GEN_W, H=GEN_H, vis_eps=1e-4):
    """the oracle's images and visibility of a generated scene under a camera given as its 16 doubles (a tuple): computed once per
    session and shared, never modified"""
    verts, faces = generated_scenes()[scene]
    img = render(verts, faces, np.array(cam_row), kind, W, H)
    vis, firm = visibility(verts, faces, np.array(cam_row), kind, W, H, vis_eps)
    for a in list(img.values()) + [vis, firm]:
        a.setflags(write=False)
    return img, vis, firm


def on_grid_camera(W, H):
    """arguments of Camera.orthographic: looking along -z with px = py = 0.5, pixel centres at (j + 0.5, H - i - 0.5)"""
    return dict(eye=(W / 2, H / 2, 16.0), target=(W / 2, H / 2, 0.0), up=(0.0, 1.0, 0.0), half_width=W / 2, half_height=H / 2, width=W, height=H)


def _exact(verts):
    v = np.asarray(verts, dtype=np.float64)
    fin = v[np.isfinite(v)]
    assert np.all(fin * 4 == np.round(fin * 4)) and np.all(np.abs(fin) <= 4096), "on-grid scenes live on quarter-integers"
    z = v[:, 2][np.isfinite(v[:, 2])]
    assert np.all(z == np.round(z)), "integer depths"
    return v


def on_grid_scenes(W, H):
    """name -> (verts, faces): every coordinate a quarter-integer, every depth an integer, so every product of the ray test is exact"""
    cover = [[-1, -1, 3], [2 * W + 2, -1, 3], [-1, 2 * H + 2, 3]]
    n = min(W, H)
    s = {}
    s["cover"] = (cover, [[0, 1, 2]])
    s["between"] = ([[0.75, 0.75, 2], [1.25, 0.75, 2], [0.75, 1.25, 2]], [[0, 1, 2]])
    s["corner"] = ([[0.5, H - 0.5, 2], [1.25, H - 0.5, 2], [0.5, H + 0.25, 2]], [[0, 1, 2]])
    s["shared_edge"] = ([[0, 0, 4], [n, 0, 4], [n, n, 4], [0, n, 4]], [[0, 1, 2], [0, 2, 3]])
    s["coplanar"] = (cover + [[-2, -2, 3], [2 * W + 1, -2, 3], [-2, 2 * H + 1, 3]], [[3, 4, 5], [0, 1, 2]])
    s["plates"] = (cover + [[0, 0, 5], [W / 2 + 0.5, 0, 5], [W / 2 + 0.5, H, 5], [0, H, 5]], [[0, 1, 2], [3, 4, 5], [3, 5, 6]])
    s["zero_area"] = ([[0, 0, 1], [2, 2, 1], [4, 4, 1], [1, 1, 1]], [[0, 1, 2], [3, 3, 3]])
    s["nan_vertex"] = (cover + [[np.nan, 0, 5], [W, 0, 5], [0, H, 5]], [[3, 4, 5], [0, 1, 2]])
    s["empty"] = ([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.zeros((0, 3)))
    s["no_hits"] = ([[W + 5, 0, 2], [W + 9, 0, 2], [W + 5, 4, 2]], [[0, 1, 2]])
    s["behind"] = ([[-1, -1, 20], [2 * W + 2, -1, 20], [-1, 2 * H + 2, 20]], [[0, 1, 2]])
    return {k: (_exact(v), np.asarray(f, dtype=np.int64).reshape(-1, 3)) for k, (v, f) in s.items()}


ON_GRID_SIZES = [(1, 1), (1, 64), (64, 1), (63, 5), (64, 4), (65, 3), (128, 96)]


def lattice(n=6, step=0.25):
    """an n x n on-grid lattice of vertices in the plane z = 2 with its faces: nearest searches between its vertices and the hit points of
    a half-integer pixel grid meet exact ties"""
    g = np.arange(n + 1) * step
    x, y = np.meshgrid(g, g, indexing="ij")
    verts = np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, 2.0)], 1)
    at = lambda i, j: i * (n + 1) + j
    faces = [[[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]] for i in range(n) for j in range(n)]
    return _exact(verts), np.array(faces, dtype=np.int64).reshape(-1, 3)
