"""Generated case tables of the mesh BVH at the sizes and inputs where csrc/bvh.hip can go wrong; shared by
tests/test_spatial_oracle.py (CPU: the oracle's tree walk against the oracle's brute force), tests/test_spatial_host.py and
tests/test_gpu_spatial.py (the device against the brute force). A case is a dict: name, meshes = [(verts, faces), ...], origins, dirs,
ray_ptr (rays per mesh), points = [per mesh [P, 3]], and ``exact`` where every coordinate lies on a coarse binary grid, so that ties on
t and on the squared distance are exact."""
import functools

import numpy as np

import labels_oracle as lo
import transfer_oracle as to

FACE_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097)         # one, two and three levels, full and one over
QUERY_COUNTS = (0, 1, 3, 4, 5, 257)                        # the ray kernels pack 4 rays per workgroup
TORUS = (64, 32)                                           # 4 096 faces
# the share of box and face tests in queries x faces on that torus (structured_case), measured with tests/spatial_oracle.py on the CPU,
# and the caps (x 1.5) that the oracle and the device must stay under
RAY_SHARE, RAY_CAP = 0.1076, 0.162
POINT_SHARE, POINT_CAP = 0.0687, 0.103


def _ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _case(name, meshes, rays, points, exact=False):
    """rays: per mesh (origins, dirs); points: per mesh [P, 3]"""
    o = np.concatenate([np.asarray(r[0], dtype=np.float64).reshape(-1, 3) for r in rays], 0)
    d = np.concatenate([np.asarray(r[1], dtype=np.float64).reshape(-1, 3) for r in rays], 0)
    return dict(name=name, meshes=[(np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(f, dtype=np.int64).reshape(-1, 3)) for v, f in meshes],
                origins=o, dirs=d, ray_ptr=_ptr([len(np.asarray(r[0]).reshape(-1, 3)) for r in rays]),
                points=[np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in points], exact=exact)


def surface_mesh(n_faces, seed):
    """the first n_faces faces of a noisy torus (labels_oracle.torus_mesh), the unused vertices kept"""
    side = 4
    while 2 * side * side < n_faces:
        side += 1
    v, f = lo.torus_mesh(side, seed=seed)
    return v, f[:n_faces]


def generic_queries(n, seed, verts):
    """n rays from inside the torus tube and from outside towards it, n points near and far from the surface"""
    rng = np.random.default_rng([0x53706174, seed, n])
    ang = rng.uniform(0, 2 * np.pi, n)
    o = np.stack([0.35 * np.cos(ang), np.zeros(n), 0.35 * np.sin(ang)], 1) + rng.uniform(-0.02, 0.02, (n, 3))
    d = rng.normal(size=(n, 3))
    far = rng.uniform(size=n) < 0.3
    o[far] = rng.uniform(-2.0, 2.0, (int(far.sum()), 3))
    d[far] = -o[far] + rng.normal(0, 0.2, (int(far.sum()), 3))
    base = verts[rng.integers(0, len(verts), n)] if len(verts) else np.zeros((n, 3))
    p = base + rng.normal(0, 0.004, (n, 3))
    p[rng.uniform(size=n) < 0.2] *= 5.0
    return (o, d), p


def grid_plate(nx=9, ny=9, twice=True):
    """a flat plate on the grid of eighths with every face present twice: exact ties everywhere"""
    v, f = to.grid_mesh(nx, ny)
    return v, (np.concatenate([f, f], 0) if twice else f)


def plate_queries(nx=9, ny=9, step=0.125):
    """rays straight down through the vertices, the edge midpoints and the cell centres of the plate, sideways rays in its plane and
    above it; points on the surface, above edges (two faces at one distance) and far away"""
    xs = np.arange(0, 2 * nx - 1) * (step / 2)
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    o = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 1.0)], 1)
    d = np.tile([0.0, 0.0, -1.0], (len(o), 1))
    side_o = np.array([[-1.0, 0.25, 0.0], [-1.0, 0.25, 0.5], [0.5, -1.0, 0.0], [0.5, 0.5, -1.0], [3.0, 0.25, 0.0]])
    side_d = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 0.5], [1.0, 0.0, 0.0]])
    pts = np.concatenate([np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1), np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.25)], 1),
                          [[8.0, -8.0, 4.0], [-16.0, 0.5, 0.0], [0.5, 0.5, -32.0]]], 0)
    return (np.concatenate([o, side_o], 0), np.concatenate([d, side_d], 0)), pts


def same_centroid_mesh(n=130, seed=3):
    """n triangles on the integer grid that all have the centroid (4, 4, 4): every Morton code ties"""
    rng = np.random.default_rng([0x43656E74, seed, n])
    A, B = rng.integers(0, 9, (n, 3)), rng.integers(0, 9, (n, 3))
    C = 12 - A - B
    v = np.stack([A, B, C], 1).reshape(-1, 3).astype(np.float64)
    return v, np.arange(3 * n).reshape(n, 3)


def box_queries():
    """the unit-eighth box [-1, 1] x [-0.5, 0.5] x [-0.25, 0.25]: rays in a box face, with zero components, a zero direction; origins
    inside, on and far outside; points at the centre, on faces, edges, corners and far away"""
    o = [[-2, 0.25, 0.25], [-2, 0.5, 0.125], [-2, 0.5, 0.25], [0, 0, 0], [0, 0, 0], [1, 0.5, 0.25], [1, 0, 0], [64, 64, 64], [64, 0.125, 0.125],
         [0, 0, 0], [-2, -2, 0], [0.5, 0.25, 4], [0, 0.75, 0], [2, 0, 0]]
    d = [[1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [-1, -0.5, -0.25], [1, 0, 0], [-1, -1, -1], [-1, 0, 0],
         [0, -1, 0], [1, 1, 0], [0, 0, -2], [1, 0, 0], [1, 0, 0]]
    p = [[0, 0, 0], [1, 0, 0], [1, 0.5, 0], [1, 0.5, 0.25], [2, 1, 0.5], [0, 0, 0.125], [0.5, 0.25, 0.25], [-64, 32, 0.5], [0, 0, 1024]]
    return (np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)), np.array(p, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def sized_cases():
    """one mesh per face count, the query counts cycled; seeded noise, nothing on a grid"""
    out = []
    for k, nf in enumerate(FACE_COUNTS):
        v, f = surface_mesh(nf, seed=k)
        rays, pts = generic_queries(QUERY_COUNTS[(k + 1) % len(QUERY_COUNTS)], k, v)
        out.append(_case(f"faces_{nf}", [(v, f)], [rays], [pts]))
    v, f = surface_mesh(200, seed=11)
    for n in QUERY_COUNTS:                                                              # every query count on a small mesh
        rays, pts = generic_queries(n, 20 + n, v)
        out.append(_case(f"queries_{n}", [(v, f)], [rays], [pts]))
    return out


@functools.lru_cache(maxsize=None)
def ragged_case():
    """a batch that mixes the face counts, with a mesh without faces, one without anything and one without queries"""
    counts, queries = (65, 0, 4097, 1, 64, 0, 4096), (5, 3, 257, 4, 0, 0, 1)
    meshes, rays, pts = [], [], []
    for k, (nf, nq) in enumerate(zip(counts, queries)):
        v, f = surface_mesh(nf, seed=30 + k)
        if k == 5:
            v = v[:0]                                                                   # neither vertices nor faces
        r, p = generic_queries(nq, 40 + k, v)
        meshes.append((v, f)); rays.append(r); pts.append(p)
    return _case("ragged", meshes, rays, pts)


@functools.lru_cache(maxsize=None)
def exact_cases():
    """everything on a coarse binary grid: the oracle's walk equals its brute force by construction"""
    out = []
    rays, pts = plate_queries()
    out.append(_case("plate_twice", [grid_plate()], [rays], [pts], exact=True))         # flat: one axis without extent
    v, f = to.grid_mesh(9, 9, seed=5)
    out.append(_case("plate_shuffled", [(v, f)], [rays], [pts], exact=True))
    v, f = same_centroid_mesh()
    o, d = lo.grid_rays(64, 1)
    out.append(_case("same_centroid", [(v, f)], [(o * 2.0, d)], [np.concatenate([v[::7], o * 2.0], 0)], exact=True))
    v, f = lo.box_mesh(1.0, 0.5, 0.25)
    rays, pts = box_queries()
    out.append(_case("box", [(v, f)], [rays], [pts], exact=True))
    v = np.tile([[0.5, 0.25, 0.125]], (3, 1))
    out.append(_case("single_point", [(v, [[0, 1, 2], [2, 1, 0]])], [([[0.5, 0.25, 1.0], [0, 0, 0]], [[0, 0, -1.0], [1, 0.5, 0.25]])],
                     [[[0.5, 0.25, 0.125], [1, 1, 1]]], exact=True))
    v, f, o, d, _ = lo.on_grid_scene()                                                  # zero-area face, NaN vertex, twins, NaN ray, zero direction
    out.append(_case("grid_scene", [(v, f)], [(o, d)], [np.concatenate([o, v[[0, 5, 11, 22]], [[np.nan, 0, 0], [np.inf, 0, 0]]], 0)], exact=True))
    v, f = lo.grid_triangles(150, 2)                                                    # random grid triangles, some degenerate
    o, d = lo.grid_rays(96, 2)
    vi = v.copy()
    vi[7, 1] = np.inf                                                                   # an infinite corner: the point rule may return another corner
    out.append(_case("grid_soup", [(v, f), (vi, f)], [(o, d), (o, d)], [o, o], exact=True))
    return out


@functools.lru_cache(maxsize=None)
def bad_face_case():
    """a face index outside its mesh in the second of three meshes: the status word, and the clamped face takes part"""
    v, f = surface_mesh(70, seed=50)
    fb = f.copy()
    fb[3, 1], fb[66, 0] = len(v) + 5, -2
    rays, pts = generic_queries(5, 51, v)
    return _case("bad_face", [(v, f), (v, fb), (v, f)], [rays, rays, rays], [pts, pts, pts])


@functools.lru_cache(maxsize=None)
def structured_case():
    """the torus of 4 096 faces with bone rays from its core circle and points scattered about its surface: where pruning is measured"""
    v, f = to.torus(*TORUS)
    pos, hier = lo.torus_chain(12, R=0.5)
    o, d, _, _ = lo.bone_rays(pos, hier, 14)
    rng = np.random.default_rng(0x546F7275)
    p = v[rng.integers(0, len(v), 256)] + rng.normal(0, 0.004, (256, 3))
    return _case("torus_4096", [(v, f)], [(o, d)], [p])


def segments_of(case, b):
    """The segments of mesh b of a case, made from its rays: a = the origin, b = the origin + 1.5 x the direction for the generic cases;
    for the exact ones b = origin + direction x 2^k with k cycling through -1, 0, 1, 2, so that some end before, some ON and some behind
    the first face. -> (a, b, skip_vertex, t_max): every third segment names the first corner of the face its ray hits first (None hit:
    vertex 0), every fifth has t_max = the ray's own nearest t over 2^k -- the hit exactly at t_max, which must not count."""
    import spatial_oracle as so
    rs = slice(case["ray_ptr"][b], case["ray_ptr"][b + 1])
    o, d = case["origins"][rs], case["dirs"][rs]
    v, f = case["meshes"][b]
    n = len(o)
    scale = 2.0 ** (np.arange(n) % 4 - 1) if case["exact"] else np.full(n, 1.5)
    with np.errstate(all="ignore"):
        end = o + d * scale[:, None]
    hit = so.brute_cast(o, d, v, f)
    fc, _ = so.clamped(v, f)
    skip = np.full(n, -1, dtype=np.int64)
    pick = (np.arange(n) % 3 == 0)
    skip[pick] = np.where(hit["face"][pick] >= 0, fc[np.maximum(hit["face"][pick], 0), 0] if len(fc) else 0, 0)
    t_max = np.ones(n)
    at = (np.arange(n) % 5 == 0) & (hit["face"] >= 0)
    with np.errstate(all="ignore"):
        t_max[at] = hit["t"][at] / scale[at]
    return o, end, skip, t_max


def all_cases():
    return sized_cases() + [ragged_case()] + exact_cases() + [bad_face_case(), structured_case()]
