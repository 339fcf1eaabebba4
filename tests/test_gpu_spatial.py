"""GPU: morig_amd/spatial.py (csrc/bvh.hip) against the numpy BRUTE FORCE of tests/spatial_oracle.py on every case of
tests/spatial_cases.py, bit for bit and with no query excused (tests/test_spatial_oracle.py shows on the CPU that the tree walk can equal
the brute force on all of them); the ``accel="bvh"`` routes of labels.py and transfer.py against the same calls without; a mesh alone
against the mesh in a batch; determinism; refit; and the amount of pruning."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import labels_oracle as lo
import spatial_cases as sc
import spatial_oracle as so
import transfer_oracle as to
from morig_amd import labels, spatial, transfer
from morig_amd.runtime import get_ops
from spatial_cases import POINT_CAP, RAY_CAP

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in sc.all_cases()}
PLAIN = [n for n in CASES if n != "bad_face"]


def same_bits(got, want):
    """equal shapes, types and bits; every NaN counts as the same NaN"""
    got, want = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()
    return got.tobytes() == want.tobytes()


def equal_bits(a, b):
    """torch.equal on the bits: the two kernels write the same NaN"""
    return a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


@functools.lru_cache(maxsize=None)
def brute_rays(name, orientation):
    """the reference of a case, computed once: per mesh dict(t, face, point, bad)"""
    c = CASES[name]
    return [so.brute_cast(c["origins"][c["ray_ptr"][b]:c["ray_ptr"][b + 1]], c["dirs"][c["ray_ptr"][b]:c["ray_ptr"][b + 1]], v, f, orientation)
            for b, (v, f) in enumerate(c["meshes"])]


@functools.lru_cache(maxsize=None)
def brute_points(name):
    c = CASES[name]
    return [so.brute_closest(c["points"][b], v, f) for b, (v, f) in enumerate(c["meshes"])]


@functools.lru_cache(maxsize=None)
def tree_of(name):
    c = CASES[name]
    return spatial.build([torch.from_numpy(v).cuda() for v, _ in c["meshes"]], [torch.from_numpy(f).cuda() for _, f in c["meshes"]])


def device_meshes(c):
    return [torch.from_numpy(v).cuda() for v, _ in c["meshes"]], [torch.from_numpy(f).cuda() for _, f in c["meshes"]]


# ------------------------------------------------------------------------------------------------------------------------- the queries
@pytest.mark.parametrize("name", PLAIN)
def test_rays_equal_the_brute_force(name):
    c = CASES[name]
    for orientation in ((0, 1, -1) if c["exact"] or len(c["origins"]) <= 8 else (0,)):
        t, face, point = spatial.cast_rays(tree_of(name), c["origins"], c["dirs"], c["ray_ptr"], orientation)
        for b, want in enumerate(brute_rays(name, orientation)):
            assert same_bits(t[b], want["t"]) and same_bits(face[b], want["face"]) and same_bits(point[b], want["point"]), (name, b, orientation)


@pytest.mark.parametrize("name", PLAIN)
def test_closest_points_equal_the_brute_force(name):
    c = CASES[name]
    got = spatial.closest_points(tree_of(name), c["points"])
    for b, want in enumerate(brute_points(name)):
        assert same_bits(got[b][0], want["face"]) and same_bits(got[b][1], want["bary"]) and same_bits(got[b][2], want["distance"]), (name, b)


@pytest.mark.parametrize("name", PLAIN)
def test_blocked_segments_equal_the_brute_force(name):
    c, bvh = CASES[name], tree_of(name)
    segs = [sc.segments_of(c, b) for b in range(len(c["meshes"]))]
    a, e, skip, t_max = (np.concatenate([s[k] for s in segs], 0) for k in range(4))
    for kw in (dict(), dict(skip_vertex=skip), dict(skip_vertex=skip, t_max=t_max)):
        got = spatial.segments_blocked(bvh, a, e, c["ray_ptr"], **kw)
        for b, (v, f) in enumerate(c["meshes"]):
            want = so.brute_blocked(segs[b][0], segs[b][1], v, f, **{k: segs[b][2 if k == "skip_vertex" else 3] for k in kw})
            assert got[b].dtype == torch.uint8 and same_bits(got[b], want["blocked"]), (name, b, list(kw))


def test_status_words_equal_those_of_the_brute_force_kernels():
    ops = get_ops()
    for name in ("bad_face", "ragged"):
        c, bvh = CASES[name], tree_of(name)
        m = bvh.mesh
        o, d = torch.from_numpy(c["origins"]).cuda(), torch.from_numpy(c["dirs"]).cuda()
        rp = torch.from_numpy(c["ray_ptr"].astype(np.int32)).cuda()
        t0, f0, p0, s0 = ops.ray_cast(o, d, rp, m.verts, m.vptr, m.faces, m.fptr, 0)
        t1, f1, p1, s1, _ = ops.bvh_ray_cast(o, d, rp, m.verts, m.vptr, m.faces, m.fptr, bvh.order, bvh.boxes, bvh.node_ptr, bvh.flags, 0)
        assert int(s0) == int(s1) == (ops.RAY_BAD_FACE if name == "bad_face" else 0)
        assert same_bits(t1, t0.cpu().numpy()) and torch.equal(f0, f1) and same_bits(p1, p0.cpu().numpy())      # the clamped face takes part
        pts = spatial.MeshBatch("test", [torch.from_numpy(p).cuda() for p in c["points"]])
        blk, n_blk = pts.blocks(ops.TRANSFER_BLOCK)
        w0, w1 = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        a0 = ops.transfer_closest(pts.verts, pts.vptr, blk, n_blk, m.verts, m.vptr, m.faces, m.fptr, w0)
        a1 = ops.bvh_closest(pts.verts, pts.vptr, m.verts, m.vptr, m.faces, m.fptr, bvh.order, bvh.boxes, bvh.node_ptr, bvh.flags, w1)
        assert int(w0) == int(w1) == (ops.TRANSFER_BAD_FACE if name == "bad_face" else ops.TRANSFER_NO_FACES)
        assert all(same_bits(x, y.cpu().numpy()) for x, y in zip(a1[:3], a0))
    with pytest.raises(ValueError, match="outside its mesh"):
        spatial.closest_points(tree_of("bad_face"), CASES["bad_face"]["points"])
    c = CASES["bad_face"]
    with pytest.raises(ValueError, match="outside its mesh"):
        spatial.segments_blocked(tree_of("bad_face"), c["origins"], c["origins"] + c["dirs"], c["ray_ptr"])


# ------------------------------------------------------------------------------------------------------------------------- the routes
@pytest.mark.parametrize("name", ["ragged", "plate_twice", "grid_scene", "faces_4097"])
def test_the_accel_routes_equal_the_plain_calls(name):
    c = CASES[name]
    verts, faces = device_meshes(c)
    for orientation in (0, 1):
        plain = labels.cast_rays(c["origins"], c["dirs"], c["ray_ptr"], verts, faces, orientation)
        tree = labels.cast_rays(c["origins"], c["dirs"], c["ray_ptr"], verts, faces, orientation, accel="bvh")
        assert all(equal_bits(a, b) for x, y in zip(plain, tree) for a, b in zip(x, y))
    skins = [to.random_skins(len(v), 4, b) for b, (v, _) in enumerate(c["meshes"])]
    plain = transfer.transfer_skins(verts, faces, skins, c["points"])
    tree = transfer.transfer_skins(verts, faces, skins, c["points"], accel="bvh")
    assert all(equal_bits(a, b) for x, y in zip(plain, tree) for a, b in zip(x, y))


def test_bone_ray_labels_with_the_tree_equal_those_without():
    v, f, pos, hier = lo.generated_scene(32)
    rig = SimpleNamespace(pos=pos, hierarchy=hier)
    (a0, fs0, d0), = labels.bone_ray_labels([v], [f], [rig])
    (a1, fs1, d1), = labels.bone_ray_labels([v], [f], [rig], accel="bvh")
    assert torch.equal(a0, a1) and same_bits(fs1, fs0.cpu().numpy()) and all(same_bits(d1[k], d0[k].cpu().numpy()) for k in d0)


# ------------------------------------------------------------------------------------------------------------------------- invariants
def test_a_mesh_alone_equals_the_mesh_in_the_batch_and_two_runs_give_the_same_bits():
    c = CASES["ragged"]
    batch = tree_of("ragged")
    t, face, point = spatial.cast_rays(batch, c["origins"], c["dirs"], c["ray_ptr"])
    near = spatial.closest_points(batch, c["points"])
    again = spatial.build(*device_meshes(c))
    assert torch.equal(again.order, batch.order) and same_bits(again.boxes, batch.boxes.cpu().numpy())
    t2, face2, point2 = spatial.cast_rays(again, c["origins"], c["dirs"], c["ray_ptr"])
    assert all(same_bits(a, b.cpu().numpy()) for x, y in ((t, t2), (face, face2), (point, point2)) for a, b in zip(x, y))
    for b in (0, 2, 6):
        v, f = c["meshes"][b]
        alone = spatial.build([torch.from_numpy(v).cuda()], [torch.from_numpy(f).cuda()])
        for k in range(4):
            rows = slice(*batch.node_ptr_host[k, b:b + 2])
            assert same_bits(alone.boxes[alone.node_ptr_host[k, 0]:alone.node_ptr_host[k, 1]], batch.boxes[rows].cpu().numpy())
        rs = slice(c["ray_ptr"][b], c["ray_ptr"][b + 1])
        ta, fa, pa = spatial.cast_rays(alone, c["origins"][rs], c["dirs"][rs], [0, rs.stop - rs.start])
        assert same_bits(ta[0], t[b].cpu().numpy()) and torch.equal(fa[0], face[b]) and same_bits(pa[0], point[b].cpu().numpy())
        na, = spatial.closest_points(alone, [c["points"][b]])
        assert all(same_bits(x, y.cpu().numpy()) for x, y in zip(na, near[b]))


def test_refit_equals_a_fresh_build_on_the_moved_mesh():
    c = CASES["faces_4097"]
    (v, f), = c["meshes"]
    rng = np.random.default_rng(7)
    moved = v * np.array([1.5, 0.5, -1.0]) + rng.normal(0, 0.01, v.shape)
    refit = tree_of("faces_4097").refit([torch.from_numpy(moved).cuda()])
    fresh = spatial.build([torch.from_numpy(moved).cuda()], [torch.from_numpy(f).cuda()])
    assert refit.order is tree_of("faces_4097").order
    for bvh in (refit, fresh):
        got, = spatial.closest_points(bvh, c["points"])
        want = so.brute_closest(c["points"][0], moved, f)
        assert same_bits(got[0], want["face"]) and same_bits(got[1], want["bary"]) and same_bits(got[2], want["distance"])
        t, face, point = spatial.cast_rays(bvh, c["origins"], c["dirs"], c["ray_ptr"])
        want = so.brute_cast(c["origins"], c["dirs"], moved, f)
        assert same_bits(t[0], want["t"]) and same_bits(face[0], want["face"]) and same_bits(point[0], want["point"])


def test_visits_show_pruning_and_equal_the_oracles_counts():
    """the caps of tests/test_spatial_oracle.py: 0.162 of Q x F for the bone rays, 0.103 for the points, on the torus of 4 096 faces"""
    c = CASES["torus_4096"]
    (v, f), = c["meshes"]
    bvh = tree_of("torus_4096")
    *_, ray_visits = spatial.cast_rays(bvh, c["origins"], c["dirs"], c["ray_ptr"], return_visits=True)
    (_, _, _, point_visits), = spatial.closest_points(bvh, c["points"], return_visits=True)
    ray_share = float(ray_visits[0].sum()) / (len(c["origins"]) * len(f))
    point_share = float(point_visits.sum()) / (len(c["points"][0]) * len(f))
    print(f"ray share {ray_share:.4f} (cap {RAY_CAP}), point share {point_share:.4f} (cap {POINT_CAP})")
    assert 0 < ray_share < RAY_CAP and 0 < point_share < POINT_CAP
    tree = so.build(v, f)
    assert same_bits(ray_visits[0], so.cast(tree, c["origins"], c["dirs"])["visits"])   # the same traversal rule, test for test
    assert same_bits(point_visits, so.closest(tree, c["points"][0])["visits"])
    a, e, skip, t_max = sc.segments_of(c, 0)
    blocked, seg_visits = spatial.segments_blocked(bvh, a, e, c["ray_ptr"], skip_vertex=skip, t_max=t_max, return_visits=True)
    want = so.blocked(tree, a, e, skip, t_max)
    assert same_bits(blocked[0], want["blocked"]) and same_bits(seg_visits[0], want["visits"])
    assert float(seg_visits[0].sum()) / (len(a) * len(f)) < RAY_CAP                     # any hit ends no later than the nearest hit
