"""A plain numpy / scipy float64 restatement of every rule of morig_amd/meshprep.py, written for reading: the
separating-axis test is vectorised over the voxels of one triangle's box, the interior is the complement of scipy.ndimage's flood of the
outside from a one-voxel pad, the edges are a Python set, the sampler thins with the farthest-point oracle of tests/point_oracle.py.
Nothing here shares code with the product. Also the scene builders of the mesh-front-end tests."""
import numpy as np
from scipy import ndimage

import point_oracle

MARGIN = 1e-9              # grid units: a voxel whose closest axis margin is below this may be left out of a generated-scene comparison


# ------------------------------------------------------------------------------------------------------------------------- normalize
def normalize(verts):
    """common_ops.normalize on an array: -> (verts, pivot, scale)"""
    v = np.array(verts, dtype=np.float64)
    lo, hi = v.min(0), v.max(0)
    scale = 1.0 / max(hi - lo)
    pivot = np.array([(lo[0] + hi[0]) / 2, lo[1], (lo[2] + hi[2]) / 2])
    v[:, 0] -= pivot[0]
    v[:, 1] -= pivot[1]
    v[:, 2] -= pivot[2]
    v *= scale
    return v, pivot, scale


# ------------------------------------------------------------------------------------------------------------------------- edges
def tpl_edge_set(faces, n_verts):
    """the set of (v, n) of get_tpl_edges"""
    edges = set()
    for f in np.asarray(faces).reshape(-1, 3):
        for a in f:
            for b in f:
                if a != b:
                    assert 0 <= a < n_verts and 0 <= b < n_verts
                    edges.add((int(a), int(b)))
    return edges


def tpl_edges(faces, n_verts, self_loops=False):
    """int64 [2, E]: the set sorted by (v, n), then one (i, i) per vertex when asked"""
    e = np.array(sorted(tpl_edge_set(faces, n_verts)), dtype=np.int64).reshape(-1, 2).T
    if self_loops:
        e = np.concatenate([e, np.tile(np.arange(n_verts, dtype=np.int64), (2, 1))], 1)
    return e


# ------------------------------------------------------------------------------------------------------------------------- voxels
def grid_coords(verts, dims):
    """-> (g float64 [V, 3], translate [3], scale): g = (p - translate) / scale * dims"""
    v = np.asarray(verts, dtype=np.float64)
    translate = v.min(0)
    scale = (v.max(0) - translate).max()
    return (v - translate) / scale * dims, translate, scale


def sat(tri, lo, hi):
    """one triangle (grid coordinates [3, 3]) against the closed unit cubes (i, j, k), lo <= (i, j, k) <= hi -> (overlap bool [X, Y, Z],
    margin float64 [X, Y, Z]: the smallest distance, over the non-zero axes, between the triangle's and the cube's intervals' ends --
    how far the nearest single-axis decision is from flipping, in grid units)"""
    idx = [np.arange(lo[c], hi[c] + 1) for c in range(3)]
    ci, cj, ck = np.meshgrid(*idx, indexing="ij")
    centre = np.stack([ci, cj, ck], -1) + 0.5
    r = tri[None, None, None, :, :] - centre[..., None, :]                            # [X, Y, Z, vertex, axis]
    e = np.stack([tri[1] - tri[0], tri[2] - tri[1], tri[0] - tri[2]])
    axes = [np.eye(3)[0], np.eye(3)[1], np.eye(3)[2], np.cross(e[0], e[1])]
    for k in range(3):
        for u in range(3):
            axes.append(np.cross(e[k], np.eye(3)[u]))
    overlap = np.ones(ci.shape, dtype=bool)
    margin = np.full(ci.shape, np.inf)
    for a in axes:
        p = (a[0] * r[..., 0] + a[1] * r[..., 1]) + a[2] * r[..., 2]                   # [X, Y, Z, vertex]
        rad = 0.5 * ((abs(a[0]) + abs(a[1])) + abs(a[2]))
        sep = np.maximum(p.min(-1) - rad, -rad - p.max(-1))                            # > 0: this axis separates
        overlap &= ~(sep > 0)
        norm = np.sqrt(a @ a)
        if norm > 0:
            margin = np.minimum(margin, np.abs(sep) / norm)
    return overlap, margin


def surface(g, faces, dims):
    """-> (surface bool [dims]^3, margin float64 [dims]^3: the closest margin of any triangle whose box holds the voxel)"""
    surf = np.zeros((dims,) * 3, dtype=bool)
    margin = np.full((dims,) * 3, np.inf)
    for f in np.asarray(faces).reshape(-1, 3):
        tri = g[f]
        lo = np.maximum(np.ceil(tri.min(0)) - 1, 0).astype(int)
        hi = np.minimum(np.floor(tri.max(0)), dims - 1).astype(int)
        if (lo > hi).any():
            continue
        o, m = sat(tri, lo, hi)
        box = tuple(slice(lo[c], hi[c] + 1) for c in range(3))
        surf[box] |= o
        margin[box] = np.minimum(margin[box], m)
    return surf, margin


def fill(surf):
    """surface voxels plus those the outside cannot reach through 6-connected non-surface voxels"""
    padded = np.pad(~surf, 1, constant_values=True)
    labels, _ = ndimage.label(padded)                                                  # the default structure: 6-connectivity
    outside = labels == labels[0, 0, 0]
    return ~outside[1:-1, 1:-1, 1:-1]


def voxelize(verts, faces, dims):
    """-> dict(data bool [dims]^3, translate, scale, surface, near: the voxels that may be left out (margin below MARGIN))"""
    g, translate, scale = grid_coords(verts, dims)
    surf, margin = surface(g, faces, dims)
    return dict(data=fill(surf), translate=translate, scale=scale, surface=surf, near=margin < MARGIN, grid=g)


# ------------------------------------------------------------------------------------------------------------------------- samples
def sample_surface(verts, faces, n_samples, oversample, seed):
    """-> (pts [n, 3], normals [n, 3], face [n], candidates dict)"""
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces).reshape(-1, 3)
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = B - A, C - A
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    cum = np.cumsum(0.5 * length)
    if not cum[-1] > 0:
        raise ValueError("no surface area")
    u = np.random.Generator(np.random.PCG64(seed)).random((n_samples * oversample, 3))
    tri = np.minimum(np.searchsorted(cum, u[:, 0] * cum[-1], side="right"), len(f) - 1)
    su = np.sqrt(u[:, 1])
    w0, w1, w2 = 1.0 - su, su * (1.0 - u[:, 2]), su * u[:, 2]
    cand = (w0[:, None] * A[tri] + w1[:, None] * B[tri]) + w2[:, None] * C[tri]
    pick = point_oracle.fps(cand.astype(np.float32), [0, len(cand)], [0, n_samples])
    chosen = tri[pick]                                                                 # never a zero-area face
    return cand[pick], n[chosen] / length[chosen][:, None], chosen, dict(cand=cand, tri=tri, pick=pick, w=np.stack([w0, w1, w2], 1))


# ------------------------------------------------------------------------------------------------------------------------- scenes
BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def box(lo, hi, skip_face=None):
    """an axis-aligned box as 8 vertices and 12 triangles (two per side; ``skip_face``: the pair to leave out, 0 .. 5)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    f = BOX_FACES if skip_face is None else np.delete(BOX_FACES, [2 * skip_face, 2 * skip_face + 1], 0)
    return v, f.copy()


def merge(*parts):
    """(verts, faces) of several meshes as one"""
    vs, fs, at = [], [], 0
    for v, f in parts:
        vs.append(np.asarray(v, dtype=np.float64))
        fs.append(np.asarray(f) + at)
        at += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def framed(parts, dims):
    """the scene plus two far single-vertex anchors at (0, 0, 0) and (dims, dims, dims), so that the frame is translate 0, scale dims
    and a vertex's coordinates ARE its grid coordinates: g = (p - 0) / dims * dims is exact for the on-grid scenes (p / dims * dims
    returns p for every p that is a multiple of 1/2 up to 96 when dims <= 96 -- asserted by the callers)"""
    v, f = merge(*parts)
    v = np.concatenate([v, [[0.0, 0.0, 0.0], [float(dims)] * 3]])
    return v, f


def uv_sphere(n_lon=32, n_lat=16, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """poles on the y axis, n_lon x n_lat faces (triangles at the poles, quads split in two elsewhere)"""
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
        for i in range(1, n_lat - 1):
            faces.append([ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)])
            faces.append([ring(i, j), ring(i + 1, j + 1), ring(i + 1, j)])
        faces.append([len(verts) - 1, ring(n_lat - 1, j), ring(n_lat - 1, j + 1)])
    return np.array(verts) + np.asarray(centre, dtype=np.float64), np.array(faces)


def torus(n_side=24, R=0.35, r=0.12):
    """the torus grid of morig_amd.synth (without its noise) and its 2 n^2 triangles"""
    u = (np.arange(n_side) / n_side) * 2.0 * np.pi
    uu, vv = np.meshgrid(u, u, indexing="ij")
    verts = np.stack([(R + r * np.cos(vv)) * np.cos(uu), r * np.sin(vv) + r, (R + r * np.cos(vv)) * np.sin(uu)], -1).reshape(-1, 3)
    idx = np.arange(n_side * n_side).reshape(n_side, n_side)
    a, b, c, d = idx, np.roll(idx, -1, 0), np.roll(np.roll(idx, -1, 0), -1, 1), np.roll(idx, -1, 1)
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)], 0)
    return verts, faces


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


# ------------------------------------------------------------------------------------------------------------------------- on-grid scenes
def snap(x, dims):
    """the nearest coordinate at or above x (a multiple of 1/4) that the frame maps onto itself: x / dims * dims == x"""
    x = float(x)
    while x / dims * dims != x:
        x += 0.5
    return x


def quad(axis, at, lo, hi):
    """a rectangle in the plane ``axis`` = at over [lo[0], hi[0]] x [lo[1], hi[1]] of the two other axes, as two triangles"""
    others = [c for c in range(3) if c != axis]
    v = np.zeros((4, 3))
    v[:, axis] = at
    for n, (a, b) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
        v[n, others[0]] = (lo[0], hi[0])[a]
        v[n, others[1]] = (lo[1], hi[1])[b]
    return v, np.array([[0, 1, 2], [0, 2, 3]])


def corridor(dims):
    """a closed container whose x-low side and inner baffles are walls in half-integer planes with a window in alternating corners (low y
    and z, then high y and z): the outside reaches the inside only by walking every cell's whole y extent, row after row, and its whole
    z extent, across the word boundaries of the bitset"""
    s = lambda x: snap(x, dims)
    c0, c1 = s(2), s(dims - 2)
    parts = [box([c0] * 3, [c1] * 3, skip_face=0)]                                      # BOX_FACES pair 0: the x = lo side
    k, x = 0, c0 + 0.5
    while x < c1 - 2:
        x = s(x)
        if k % 2 == 0:
            cut = s(c0 + 3.5)
            parts += [quad(0, x, (cut, c0), (c1, c1)), quad(0, x, (c0, cut), (cut, c1))]
        else:
            cut = s(c1 - 4.5)
            parts += [quad(0, x, (c0, c0), (cut, c1)), quad(0, x, (cut, c0), (c1, cut))]
        k, x = k + 1, x + 3.0
    return parts


def on_grid_scenes(dims):
    """name -> (verts, faces) in units where the frame is translate 0, scale dims (two vertices in no face sit at the grid's corners), so
    that every vertex has the integer, half- or quarter-integer grid coordinates it is written with and every quantity of the
    separating-axis test is exact. Only the scenes that fit ``dims`` are returned."""
    d, s = dims, (lambda x: snap(x, dims))
    scenes = {}
    scenes["grid_cube"] = [box([0.0] * 3, [float(d)] * 3)]                             # touches all six grid faces
    scenes["spanning_triangle"] = [(np.array([[0.0, 0.0, 0.0], [d, d, 0.0], [0.0, d, d]], dtype=np.float64), np.array([[0, 1, 2]]))]
    for i in range(d // 2, d):                                                         # the first voxel whose quarter points the frame keeps
        inside = np.array([[i + 0.25, i + 0.25, i + 0.25], [i + 0.75, i + 0.25, i + 0.5], [i + 0.25, i + 0.75, i + 0.75]])
        if all(x / d * d == x for x in inside.reshape(-1)):
            scenes["triangle_in_one_voxel"] = [(inside, np.array([[0, 1, 2]]))]
            break
    if d >= 8:
        q = d // 4
        a, b = s(q), s(d - q)
        scenes["zero_area_triangles"] = [(np.array([[a, a, a], [s(a + 2), s(a + 2), s(a + 2)], [s(a + 4), s(a + 4), s(a + 4)], [b, a, a]]),
                                          np.array([[0, 1, 2], [0, 3, 3], [1, 1, 1]]))]       # collinear; two equal corners; a point
        scenes["closed_box"] = [box([a] * 3, [b] * 3)]
        scenes["open_box"] = [box([a] * 3, [b] * 3, skip_face=3)]
        scenes["overlapping_boxes"] = [box([a] * 3, [s(d // 2 + 2)] * 3), box([s(d // 2 - 2)] * 3, [b] * 3)]
        scenes["disjoint_boxes"] = [box([s(1)] * 3, [s(q)] * 3), box([s(d - q)] * 3, [s(d - 1)] * 3)]
        m = s(d // 2)
        scenes["plate_in_a_grid_plane"] = [quad(2, m, (a, a), (b, b))]                  # touching: both neighbouring layers
        scenes["thin_plate"] = [box([a, a, m], [b, b, s(m + 0.5)])]
    if d >= 16:
        q = d // 4
        a, b = s(q), s(d - q)
        scenes["nested_boxes"] = [box([a] * 3, [b] * 3), box([s(a + 2)] * 3, [s(b - 3)] * 3)]
    if d >= 31:
        scenes["corridor"] = corridor(d)
    out = {}
    for name, parts in scenes.items():
        v, f = framed(parts, d)
        g = v / d * d
        assert np.array_equal(g, v) and np.array_equal(v * 4, np.round(v * 4)), name
        out[name] = (v, f)
    return out
