"""Generated case tables of the two visibility rules on the mesh BVH at the sizes and inputs where the kernels of
csrc/bvh.hip can go wrong; shared by tests/test_visibility_oracle.py (CPU: the oracle's walk against the oracle's brute force) and
tests/test_gpu_visibility.py (the device against the brute-force kernels and the oracle).

A SCAN case is a dict: name, faces = [per mesh [F, 3]], views = [(verts [V, 3], mesh, camera)], vis_eps, with a camera as
(kind name, the keyword arguments of morig_amd.scan.Camera.orthographic / .pinhole). A BONE case is a dict: name, meshes =
[(pos [V, 3], bones [nb, 6], tri_pos [T, 3], tri_faces [F, 3])]."""
import functools

import numpy as np

import labels_oracle as lo
import scan_oracle as sco
import spatial_cases as sc
import transfer_oracle as to

SCAN_FACE_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097)    # one, two and three levels, full and one over
SCAN_VERTEX_COUNTS = (0, 1, 63, 64, 65, 257)               # the kernel packs 4 vertices per workgroup
BONE_FACE_COUNTS = (0, 1, 255, 257, 1922, 4097)
BONE_COUNTS = (1, 2, 5, 33, 3, 7)
TORUS = (64, 32)                                           # 4 096 faces
W, H = sco.GEN_W, sco.GEN_H
DYADIC_EPS = 0.5
# the share of box and face tests in queries x faces, measured with tests/visibility_oracle.py on the CPU (tests/test_visibility_oracle.py
# prints them), and the caps (x 1.5, as tests/spatial_cases.py caps its own) that the oracle and the device must stay under
SCAN_SHARE = {"orthographic": 0.0762, "pinhole": 0.0810}   # the 64 x 32 torus under the two generated cameras
SCAN_CAP = {"orthographic": 0.114, "pinhole": 0.122}
STALE_SHARE, STALE_CAP = 0.0788, 0.118                     # that torus bent by 70 degrees, its faces in the order of the rest pose
BONE_SHARE, BONE_CAP = 0.1334, 0.2                          # the 48 x 48 torus as its own occluder, six bones in its tube


def cameras(w=W, h=H):
    return [(k, kw) for k, kw in sco.generated_cameras(w, h).items()]


def camera_of(spec):
    """the product's Camera of a case's camera (its ``row()`` is what the oracle takes, its ``kind`` the oracle's kind)"""
    from morig_amd.scan import Camera
    kind, kw = spec
    return getattr(Camera, kind)(**kw)


def _scan(name, faces, views, vis_eps=1e-4):
    return dict(name=name, faces=[np.asarray(f, dtype=np.int64).reshape(-1, 3) for f in faces],
                views=[(np.asarray(v, dtype=np.float64).reshape(-1, 3), int(m), cam) for v, m, cam in views], vis_eps=float(vis_eps))


# ------------------------------------------------------------------------------------------------------------------------- scan cases
def strip_mesh(nv, nf, seed):
    """nv vertices along a noisy helix about the view axis and nf faces (k, k + a, k + b) mod nv with small a < b: thin triangles that
    cover one another from every side; with nv == 1 every face is the point itself"""
    rng = np.random.default_rng([0x56697369, seed, nv, nf])
    k = np.arange(nv)
    ang = 2.0 * np.pi * k * (5.0 / max(nv, 1)) + rng.uniform(0, 0.05, nv)
    v = np.stack([0.6 * np.cos(ang), 0.6 * np.sin(ang), -0.5 + k / max(nv, 1)], 1) + rng.normal(0, 0.01, (nv, 3))
    j = np.arange(nf)
    if nv == 0:
        return v, np.zeros((0, 3), dtype=np.int64)
    f = np.stack([j % nv, (j + 1 + j // nv) % nv, (j + 2 + 2 * (j // nv)) % nv], 1)
    return v, f.astype(np.int64)


def bent(verts, degrees=70.0):
    """an articulated bend of the torus of transfer_oracle.torus: the half with x > 0 turns about the z axis through the origin"""
    a = np.radians(degrees) * np.clip(verts[:, 0] / 0.3, 0.0, 1.0)
    out = verts.copy()
    out[:, 0] = np.cos(a) * verts[:, 0] - np.sin(a) * verts[:, 1]
    out[:, 1] = np.sin(a) * verts[:, 0] + np.cos(a) * verts[:, 1]
    return out


@functools.lru_cache(maxsize=None)
def scan_sized_cases():
    out, cams = [], cameras()
    for k, nf in enumerate(SCAN_FACE_COUNTS):                                           # a surface of every face count, its vertices the queries
        v, f = sc.surface_mesh(nf, seed=60 + k)
        out.append(_scan(f"faces_{nf}", [f], [(v * 1.6, 0, cams[k % 2])]))
    for k, nv in enumerate(SCAN_VERTEX_COUNTS):
        v, f = strip_mesh(nv, 200 if nv else 0, seed=k)
        out.append(_scan(f"verts_{nv}", [f], [(v, 0, cams[(k + 1) % 2])]))
    return out


@functools.lru_cache(maxsize=None)
def scan_batch_case():
    """three views of two meshes with view_mesh = [1, 0, 1] and a third mesh that no view draws; the two views of mesh 1 in two poses"""
    v0, f0 = strip_mesh(65, 130, seed=20)
    v1, f1 = sc.surface_mesh(300, seed=21)
    v2, f2 = strip_mesh(9, 7, seed=22)
    cams = cameras()
    return _scan("views_of_two_meshes", [f0, f1, f2], [(v1 * 1.6, 1, cams[0]), (v0, 0, cams[1]), (bent(v1 * 1.6, 40.0), 1, cams[1])])


def strict_scene():
    """An orthographic camera at z = 16 looking down -z (scan_oracle.on_grid_camera): a vertex at depth 0 has len = 16. Vertex 0 lies under a
    plate at z = 1/2: t len == len - 1/2 exactly, which must NOT block under vis_eps = 1/2 and blocks under 0. Vertex 1 lies under a plate
    at z = 1: blocked under both. Vertex 2 lies IN a plate at z = 0 that does not name it: t == 1 exactly, never a block. Vertex 3 is a
    corner of the plate above it at its own depth and a twin of vertex 4 at the same place, which that plate does not name (t == 1 again)."""
    v = [[1.25, 1.25, 0], [5.25, 1.25, 0], [9.25, 1.25, 0], [13, 1, 0], [13, 1, 0],
         [0, 0, 0.5], [3, 0, 0.5], [0, 3, 0.5], [4, 0, 1], [7, 0, 1], [4, 3, 1], [8, 0, 0], [11, 0, 0], [8, 3, 0], [15, 1, 0], [13, 3, 0]]
    f = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [3, 14, 15]]
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64)


STRICT_WANT = {0.0: (0, 0, 1, 1, 1), DYADIC_EPS: (1, 0, 1, 1, 1)}                       # vis of the vertices 0 .. 4 of strict_scene


@functools.lru_cache(maxsize=None)
def scan_grid_cases():
    """scan_oracle.on_grid_scenes and strict_scene under vis_eps = 0 and a dyadic vis_eps: every product exact, the boundary decided exactly"""
    out = []
    w, h = 16, 8
    cam = ("orthographic", sco.on_grid_camera(w, h))
    for eps in (0.0, DYADIC_EPS):
        for name, (v, f) in sco.on_grid_scenes(w, h).items():
            out.append(_scan(f"grid_{name}_eps{eps}", [f], [(v, 0, cam)], eps))
        v, f = strict_scene()
        out.append(_scan(f"strict_eps{eps}", [f], [(v, 0, cam)], eps))
    return out


@functools.lru_cache(maxsize=None)
def scan_generated_cases():
    """both cameras on the generated torus and triangles of scan_oracle: where the restated brute force meets scan_oracle.visibility"""
    return [_scan(f"{scene}_{cam[0]}", [f], [(v, 0, cam)]) for scene, (v, f) in sco.generated_scenes().items() for cam in cameras()]


@functools.lru_cache(maxsize=None)
def scan_special_cases():
    out, cams = [], cameras()
    v, f = sc.surface_mesh(300, seed=23)
    v = v * 1.6
    out.append(_scan("outside_the_frustum", [f], [(v + [0.9, 0.0, 0.0], 0, cams[0]), (v * [1.0, 1.0, -1.0] + [0.0, 0.0, 3.2], 0, cams[1])]))
    nan = v.copy()
    nan[17, 1] = np.nan
    out.append(_scan("nan_vertex", [f], [(nan, 0, cams[0])]))
    return out


@functools.lru_cache(maxsize=None)
def scan_bad_face_case():
    v, f = sc.surface_mesh(70, seed=24)
    fb = f.copy()
    fb[3, 1], fb[66, 0] = len(v) + 5, -2
    return _scan("bad_face", [fb], [(v * 1.6, 0, cameras()[0])])


@functools.lru_cache(maxsize=None)
def scan_torus_cases():
    """the 64 x 32 torus under both cameras, where pruning is measured; and ordered on its rest pose, boxed on a strongly bent one"""
    v, f = to.torus(*TORUS)
    v = v @ sco.rotation(5).T
    out = [_scan(f"torus_4096_{cam[0]}", [f], [(v, 0, cam)]) for cam in cameras()]
    out.append(_scan("torus_4096_stale", [f], [(v, 0, cameras()[0]), (bent(v), 0, cameras()[0])]))
    return out


def scan_cases():
    return (scan_sized_cases() + [scan_batch_case()] + scan_grid_cases() + scan_generated_cases() + scan_special_cases() + scan_torus_cases())


# ------------------------------------------------------------------------------------------------------------------------- bone cases
def chain_bones(nb, seed, R=0.35, r=0.12):
    """nb bones inside the tube of labels_oracle.torus_mesh, their joints off the core circle by up to 0.4 r so that no ray runs along a
    mesh edge; every seventh bone has zero length"""
    rng = np.random.default_rng([0x426F6E65, seed, nb])
    ang = 2.0 * np.pi * (np.arange(nb + 1) + rng.uniform(0.1, 0.4, nb + 1)) / (nb + 1)
    j = np.stack([R * np.cos(ang), np.zeros(nb + 1), R * np.sin(ang)], 1) + rng.uniform(-0.4 * r, 0.4 * r, (nb + 1, 3)) / np.sqrt(3.0)
    bones = np.concatenate([j[:-1], j[1:]], 1)
    bones[6::7, 3:6] = bones[6::7, 0:3]
    return bones


def _bone(name, meshes):
    return dict(name=name, meshes=[(np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 6),
                                    np.asarray(t, dtype=np.float64).reshape(-1, 3), np.asarray(f, dtype=np.int64).reshape(-1, 3))
                                   for p, b, t, f in meshes])


def bone_mesh(nf, nb, seed, n_pos=48):
    """an occluder of nf faces of the noisy torus, nb bones in its tube, and n_pos vertices to look at: corners of the occluder (the ray
    ends on a corner), midpoints of its edges (on an edge), points outside it and, first of all, a point ON the first bone (a ray of
    length zero)"""
    rng = np.random.default_rng([0x426F6E66, seed, nf])
    v, f = sc.surface_mesh(nf, seed=seed)
    bones = chain_bones(nb, seed)
    some = v[rng.integers(0, len(v), n_pos // 3)]
    mid = 0.5 * (v[f[rng.integers(0, len(f), n_pos // 3), 0]] + v[f[rng.integers(0, len(f), n_pos // 3), 1]]) if len(f) else some
    far = some * 1.3 + rng.normal(0, 0.02, some.shape)
    return np.concatenate([bones[:1, 0:3], some, mid, far], 0), bones, v, f


@functools.lru_cache(maxsize=None)
def bone_sized_cases():
    return [_bone(f"occluder_{nf}", [bone_mesh(nf, BONE_COUNTS[k], 70 + k)]) for k, nf in enumerate(BONE_FACE_COUNTS)]


@functools.lru_cache(maxsize=None)
def bone_grid_cases():
    """on a coarse binary grid: rays lying exactly in a face's plane (det == 0), a bone boxed in by a cube (an all-invisible column next
    to a visible one), and a vertex without any occluder vertex"""
    plate_v, plate_f = to.grid_mesh(5, 5, step=0.5)                                     # the plane z = 0 over [0, 2]^2
    in_plane = np.array([[3.0, 0.5, 0.0], [3.0, 1.0, 0.0], [-1.0, 1.25, 0.0], [1.0, 3.0, 0.0], [0.75, 0.25, 1.0], [0.75, 0.25, -1.0]])
    bones = np.array([[-2.0, 0.5, 0.0, -2.0, 1.5, 0.0], [1.0, 1.0, 2.0, 1.0, 1.0, 2.0], [1.0, 1.0, -2.0, 1.0, 1.5, -2.0]])
    cube_v, cube_f = lo.box_mesh(1.0, 0.5, 0.25)
    outside = np.array([[4.0, 0.0, 0.0], [0.0, 3.0, 0.5], [-2.0, -2.0, -2.0], [0.5, 0.25, 0.125], [1.0, 0.5, 0.25]])
    boxed = np.array([[-0.5, 0.0, 0.0, 0.5, 0.0, 0.0], [3.0, 3.0, 3.0, 3.0, 3.0, 4.0]])
    return [_bone("rays_in_a_plane", [(in_plane, bones, plate_v, plate_f)]),
            _bone("boxed_in", [(outside, boxed, cube_v, cube_f)]),
            _bone("no_occluder_vertices", [(outside, boxed, np.zeros((0, 3)), np.zeros((0, 3)))])]


@functools.lru_cache(maxsize=None)
def bone_nan_case():
    p, b, v, f = bone_mesh(255, 3, 81)
    v = v.copy()
    v[f[5, 1], 2] = np.nan                                                              # the faces around this vertex are never hit
    p = p.copy()
    p[3, 0] = np.nan                                                                    # and this vertex sees nothing
    return _bone("nan", [(p, b, v, f)])


@functools.lru_cache(maxsize=None)
def bone_ragged_cases():
    """a batch that mixes the occluder sizes and the bone counts, in two orders"""
    meshes = [bone_mesh(nf, nb, 90 + k, n_pos=12 + 9 * k) for k, (nf, nb) in enumerate(((257, 33), (0, 1), (4097, 2), (1, 5), (64, 8)))]
    return [_bone("ragged", meshes), _bone("ragged_reversed", meshes[::-1])]


@functools.lru_cache(maxsize=None)
def bone_generated_case():
    """the noisy torus as its own occluder, 4 096 faces, every vertex looked at from six bones in the tube: where the restated brute force
    meets skin_oracle.ray_caster and where pruning is measured"""
    v, f = lo.torus_mesh(48, seed=3)                                                    # 4 608 faces
    return _bone("torus_own_occluder", [(v[::9], chain_bones(6, 3)[:6], v, f)])


def bone_cases():
    return bone_sized_cases() + bone_grid_cases() + [bone_nan_case()] + bone_ragged_cases() + [bone_generated_case()]
