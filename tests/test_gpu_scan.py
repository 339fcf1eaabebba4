"""GPU: morig_amd/scan.py (csrc/scan.hip) against tests/scan_oracle.py -- on-grid scenes where every product of the ray test is exact
(whole images, bit for bit, nothing excused: this is where touching, ties and the key rule are tested), pinhole edge cases, generated
scenes (a pixel or vertex is excused only where the oracle's own margin is under 1e-9, and tests/test_scan_oracle.py shows on the CPU
that this is under a thousandth), ragged batches, determinism, the refusals, and the results going through the stages that consume
them."""
import numpy as np
import pytest
import torch

import scan_oracle as so
from morig_amd import losses, native, playback, scan, tracking
from morig_amd.formats import Rig

pytestmark = pytest.mark.gpu


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def same_bits(got, want):
    got, want = host(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def images_equal(got, want):
    depth, face, point = got
    return same_bits(depth, want["depth"]) and same_bits(face, want["face"]) and same_bits(point, want["point"])


# ------------------------------------------------------------------------------------------------------------------------- on grid
@pytest.mark.parametrize("size", so.ON_GRID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_on_grid_scenes_equal_the_oracle_bit_for_bit(size):
    W, H = size
    cam = scan.Camera.orthographic(**so.on_grid_camera(W, H))
    assert cam.px == 0.5 and cam.py == 0.5
    scenes = so.on_grid_scenes(W, H)
    names = list(scenes)
    out = scan.render([scenes[n][0] for n in names], [scenes[n][1] for n in names], [cam] * len(names))
    hits = {}
    for n, got in zip(names, out):
        want = so.render(scenes[n][0], scenes[n][1], cam.row(), cam.kind, W, H)
        assert got[0].is_cuda and tuple(got[0].shape) == (H, W) and images_equal(got, want), n
        hits[n] = want["face"]
    assert (hits["cover"] == 0).all() and (hits["coplanar"] == 0).all() and (hits["nan_vertex"] == 1).all()
    for n in ("between", "zero_area", "empty", "no_hits", "behind"):
        assert (hits[n] == -1).all(), n
    assert (hits["corner"] >= 0).sum() == 1 and hits["corner"][0, 0] == 0                  # the corner on the centre of pixel (0, 0)
    diag = hits["shared_edge"][H - 1 - np.arange(min(W, H)), np.arange(min(W, H))]          # centres (k + 0.5, k + 0.5): on the shared edge
    assert (diag == 0).all()
    if min(W, H) > 1:
        assert set(np.unique(hits["shared_edge"])) >= {0, 1} and set(np.unique(hits["plates"])) == {0, 1, 2}
        assert (hits["plates"][:, 0] > 0).all() and (hits["plates"][:, -1] == 0).all()
    pts = scan.scan_meshes([scenes["plates"][0]], [scenes["plates"][1]], [cam])[0]
    flat = hits["plates"].reshape(-1)
    assert same_bits(pts.pixel, np.arange(W * H, dtype=np.int64)) and same_bits(pts.face, flat.astype(np.int64))


def test_one_triangle_covering_256_x_256():
    cam = scan.Camera.orthographic(**so.on_grid_camera(256, 256))
    v, f = so.on_grid_scenes(256, 256)["cover"]
    got, = scan.render([v], [f], [cam])
    assert images_equal(got, so.render(v, f, cam.row(), cam.kind, 256, 256)) and bool((got[1] == 0).all()) and bool((got[0] == 13.0).all())


# ------------------------------------------------------------------------------------------------------------------------- generated
def firm_compare(got, want, what):
    """faces equal wherever the oracle's margin is at least MARGIN; depth and point within 1e-12 where the faces agree"""
    depth, face, point = (host(t) for t in got)
    firm = want["margin"] >= so.MARGIN
    hits = int((want["face"] >= 0).sum())
    assert (~firm).sum() <= 0.001 * hits, what
    assert np.array_equal(face[firm], want["face"][firm]), what
    agree = (face == want["face"]) & (face >= 0)
    dd, dp = np.abs(depth[agree] - want["depth"][agree]).max(initial=0.0), np.abs(point[agree] - want["point"][agree]).max(initial=0.0)
    bit_equal = depth[agree].tobytes() == want["depth"][agree].tobytes() and point[agree].tobytes() == want["point"][agree].tobytes()
    print(f"{what}: {hits} hit pixels, {int((~firm).sum())} left out, max |depth diff| {dd:.3g}, max |point diff| {dp:.3g}, bit-equal {bit_equal}")
    assert dd <= 1e-12 and dp <= 1e-12 and np.all(np.isinf(depth[face < 0])), what
    return hits


def pinhole_edge_scenes():
    tri = lambda *p: (np.array(p, dtype=np.float64), np.array([[0, 1, 2]]))
    return {"behind_the_eye": tri([-0.5, -0.4, 3.1], [0.6, -0.3, 3.4], [0.1, 0.7, 3.2]),
            "crossing_near": tri([-0.7, -0.5, 1.0], [0.8, -0.45, 1.2], [0.05, 0.3, 2.45]),
            "box_leaves_the_image": tri([-40.0, -31.0, -3.0], [43.0, -29.0, -2.5], [1.0, 52.0, -3.5]),
            "mixed": (np.array([[-40.0, -31.0, -3.0], [43.0, -29.0, -2.5], [1.0, 52.0, -3.5], [-0.7, -0.5, 1.0], [0.8, -0.45, 1.2], [0.05, 0.3, 2.45],
                                [-0.5, -0.4, 3.1], [0.6, -0.3, 3.4], [0.1, 0.7, 3.2]]), np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]]))}


def test_pinhole_edge_cases():
    W, H = 65, 47
    cam = scan.Camera.pinhole((0.05, 0.02, 2.5), (0.0, 0.0, 0.0), (0, 1, 0), 50.0, W, H, near=0.25)
    scenes = pinhole_edge_scenes()
    out = scan.render([s[0] for s in scenes.values()], [s[1] for s in scenes.values()], [cam] * len(scenes))
    hits = {}
    for (name, (v, f)), got in zip(scenes.items(), out):
        want = so.render(v, f, cam.row(), cam.kind, W, H)
        hits[name] = firm_compare(got, want, name)
        assert np.all(host(got[0])[host(got[1]) >= 0] > 0.25)                            # nothing at or in front of the near plane
    assert hits["behind_the_eye"] == 0 and hits["box_leaves_the_image"] == W * H and 0 < hits["crossing_near"] < W * H


@pytest.mark.parametrize("scene", ["torus", "triangles"])
def test_generated_scenes_under_both_cameras(scene):
    W, H = so.GEN_W, so.GEN_H
    verts, faces = so.generated_scenes()[scene]
    cams = [getattr(scan.Camera, k)(**kw) for k, kw in so.generated_cameras(W, H).items()]
    images = scan.render([verts, verts], [faces], cams, view_mesh=[0, 0])
    scans = scan.scan_meshes([verts, verts], [faces], cams, view_mesh=[0, 0], corr_radius=0.05)
    thin = scan.scan_meshes([verts, verts], [faces], cams, view_mesh=[0, 0], corr_radius=0.05, n_pts=300)
    for cam, got, sc, th in zip(cams, images, scans, thin):
        img, vis, firm = so.generated_reference(scene, tuple(cam.row()), cam.kind)
        firm_compare(got, img, f"{scene} / kind {cam.kind}")
        mine = host(sc.vismask)
        assert sc.vismask.dtype == torch.uint8 and (~firm).sum() <= 0.001 * len(vis) and np.array_equal(mine[firm], vis[firm])
        assert same_bits(th.vismask, mine)
        for s, n_pts in ((sc, None), (th, 300)):                                             # given the device's own images and mask
            want = so.scan_from_images(verts, host(got[1]), host(got[2]), mine, n_pts, 0.05)
            for name in ("pts", "pixel", "face", "corr_v2p", "corr_p2v"):
                assert same_bits(getattr(s, name), want[name]), (scene, cam.kind, n_pts, name)
            assert len(want["corr_v2p"]) > 20 and len(want["corr_p2v"]) > 20


def test_nearest_ties_on_a_lattice_and_a_view_that_sees_no_vertex():
    verts, faces = so.lattice(6, 0.25)                                                     # vertices every quarter, pixel centres every half
    cam = scan.Camera.orthographic(**so.on_grid_camera(2, 2))
    away = scan.Camera.orthographic((1.0, 1.0, 16.0), (1.0, 1.0, 32.0), (0, 1, 0), 1.0, 1.0, 2, 2)      # looks away: sees nothing
    lit, dark = scan.scan_meshes([verts, verts], [faces], [cam, away], view_mesh=[0, 0], corr_radius=0.36)
    got, = scan.render([verts], [faces], [cam])
    want = so.scan_from_images(verts, host(got[1]), host(got[2]), host(lit.vismask), None, 0.36)
    assert bool(lit.vismask.all()) and lit.pts.shape[0] == 4
    for name in ("pts", "pixel", "face", "corr_v2p", "corr_p2v"):
        assert same_bits(getattr(lit, name), want[name]), name
    d = np.linalg.norm(verts[:, None] - host(lit.pts)[None], axis=2)
    assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() >= 8               # vertices at equal distance from two points
    assert not bool(dark.vismask.any()) and dark.pts.shape == (0, 3) and dark.corr_v2p.shape == (0, 2) and dark.corr_p2v.shape == (0, 2)


# ------------------------------------------------------------------------------------------------------------------------- batches
def batch_views():
    tv, tf = so.torus(n=10)
    rv, rf = so.random_triangles(40)
    turned = tv @ so.rotation(21).T
    o = lambda W, H: scan.Camera.orthographic((0.3, 0.4, 3.0), (0, 0, 0), (0, 1, 0), 1.1, 1.1 * H / W, W, H)
    p = lambda W, H: scan.Camera.pinhole((0.5, 0.7, 2.6), (0, 0.05, 0), (0.1, 1, 0), 42.0, W, H)
    empty = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    meshes = [(tv, tf), (rv, rf), empty, (tv + [40.0, 0, 0], tf)]
    #        (vertices, mesh, camera): two frames of mesh 0, another mesh, an empty one, one out of sight; four image sizes
    views = [(tv, 0, o(33, 17)), (rv, 1, p(64, 40)), (turned, 0, p(31, 65)), (empty[0], 2, o(8, 8)), (meshes[3][0], 3, o(33, 17))]
    return meshes, views


def run_views(meshes, views, **kw):
    faces = [m[1] for m in meshes]
    call = lambda fn, **k: fn([v[0] for v in views], faces, [v[2] for v in views], view_mesh=[v[1] for v in views], **k)
    return call(scan.render), call(scan.scan_meshes, corr_radius=0.06, **kw)


def flatten(images, scans):
    return [host(t) for img in images for t in img] + [host(t) for s in scans for t in s]


def test_a_ragged_batch_equals_the_single_runs_in_any_order_and_twice():
    meshes, views = batch_views()
    images, scans = run_views(meshes, views)
    assert [int(s.pts.shape[0]) > 0 for s in scans] == [True, True, True, False, False]
    for v, view in enumerate(views):
        (img,), (sc,) = run_views(meshes, [view])
        for a, b in zip(flatten([images[v]], [scans[v]]), flatten([img], [sc])):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), v
    order = [4, 2, 0, 3, 1]
    images2, scans2 = run_views(meshes, [views[k] for k in order])
    for k, v in enumerate(order):
        for a, b in zip(flatten([images[v]], [scans[v]]), flatten([images2[k]], [scans2[k]])):
            assert a.tobytes() == b.tobytes(), v
    again = flatten(*run_views(meshes, views))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flatten(images, scans), again))
    small = flatten(*run_views(meshes, views, key_budget=8 * 64 * 40))                     # the same views in chunks
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flatten(images, scans), small))


def test_vertex_counts_at_the_segment_edges_equal_the_views_alone_and_the_oracle():
    counts = [0, 1, 256, 0, 257, 255, 0]                       # empty views in front, between and behind; a full workgroup, one row more, one less
    rng, W = np.random.default_rng(11), 24
    cam = scan.Camera.orthographic((0.1, 0.2, 3.0), (0, 0, 0), (0, 1, 0), 1.2, 1.2, W, W)
    meshes = [(rng.uniform(-1, 1, (n, 3)), np.stack([rng.permutation(n)[:3] for _ in range(30)]) if n >= 3 else np.zeros((0, 3), dtype=np.int64))
              for n in counts]
    views = [(v, m, cam) for m, (v, _) in enumerate(meshes)]
    images, scans = run_views(meshes, views)
    for k, view in enumerate(views):
        (img,), (sc,) = run_views(meshes, [view])
        for a, b in zip(flatten([images[k]], [scans[k]]), flatten([img], [sc])):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
        vis, firm = so.visibility(*meshes[k], cam.row(), cam.kind, W, W, 1e-4)
        mine = host(scans[k].vismask)
        assert mine.shape == (counts[k],) and (~firm).sum() <= 0.001 * len(vis) and np.array_equal(mine[firm], vis[firm]), k
        want = so.scan_from_images(meshes[k][0], host(images[k][1]), host(images[k][2]), mine, None, 0.06)
        for name in ("pts", "pixel", "face", "corr_v2p", "corr_p2v"):
            assert same_bits(getattr(scans[k], name), want[name]), (k, name)
    assert max(int(s.pts.shape[0]) for s in scans) > 256 and 0 < int(scans[4].vismask.sum()) < 257


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    verts, faces = so.torus(n=8)
    cam = scan.Camera.orthographic((0, 0, 3), (0, 0, 0), (0, 1, 0), 1.1, 1.1, 32, 32)
    bad = faces.copy()
    bad[5, 2] = len(verts)
    with pytest.raises(ValueError, match="a face names a vertex outside its mesh"):
        scan.render([verts], [bad], [cam])
    with pytest.raises(ValueError, match="a face names a vertex outside its mesh"):
        scan.scan_meshes([verts, verts], [faces, bad], [cam, cam])
    for w in (0, 1025):
        with pytest.raises(ValueError, match="supported are 1 .. 1024"):
            scan.Camera.orthographic((0, 0, 3), (0, 0, 0), (0, 1, 0), 1, 1, w, 32)
        ops = native.get_ops()                                                             # the library refuses it before any launch
        i32, i64 = (lambda a: dev(a, torch.int32)), (lambda a: dev(a, torch.int64))
        with pytest.raises(native.MorigNativeError, match="morig_scan_raster"):
            ops.scan_raster(dev(verts), i32([0, len(verts)]), i32(faces), i32([0, len(faces)]), i32([len(verts)]), dev(cam.row()[None]),
                            i32([[0, max(w, 1), 32, 0]]), i64([0, max(w, 1) * 32]), i64([0, len(faces)]), min(w, 32), max(w, 32), max(w, 1) * 32,
                            len(faces))
    hits = int((scan.render([verts], [faces], [cam])[0][1] >= 0).sum())
    with pytest.raises(ValueError, match=f"view 0 has {hits} hits, fewer than n_pts = {hits + 1}"):
        scan.scan_meshes([verts], [faces], [cam], n_pts=hits + 1)
    assert scan.scan_meshes([verts], [faces], [cam], n_pts=hits)[0].pts.shape[0] == hits
    cover = scan.Camera.orthographic(**so.on_grid_camera(256, 256))
    cv, cf = so.on_grid_scenes(256, 256)["cover"]
    with pytest.raises(ValueError, match="view 0 has 65536 hits: thinning to n_pts takes at most 32768"):
        scan.scan_meshes([cv], [cf], [cover], n_pts=256)


# ------------------------------------------------------------------------------------------------------------------------- consumers
def test_a_replayed_rig_goes_through_the_scan_into_its_consumers():
    verts, faces = so.torus(n=12, seed=2)
    V, T, n_pts = len(verts), 3, 256
    joints = np.array([[-0.5, 0, 0], [0.0, 0, 0], [0.5, 0, 0]])
    w = np.exp(-8.0 * np.linalg.norm(verts[:, None] - joints[None], axis=2) ** 2)
    w[w < 0.05] = 0.0
    w[np.arange(V), np.argmax(np.exp(-np.linalg.norm(verts[:, None] - joints[None], axis=2)), axis=1)] += 0.1
    rig = Rig.from_arrays(joints, [-1, 0, 1], 0, skins=w / w.sum(axis=1, keepdims=True))
    ang = np.array([[0.0, 0.0, 0.0], [0.0, 0.15, 0.3], [0.0, -0.2, -0.35]])                  # per joint and frame, about z
    quats = np.stack([np.zeros((3, T)), np.zeros((3, T)), np.sin(ang / 2), np.cos(ang / 2)], 2)
    traj, = playback.skin_trajectory([rig], [dev(verts)], [dev(quats)])
    assert tuple(traj.shape) == (V, T, 3)
    cam = scan.Camera.pinhole((0.3, 0.5, 2.8), (0, 0, 0), (0, 1, 0), 40.0, 96, 96)
    (pts_traj, vismask, v2p, p2v), = scan.scan_trajectory([traj], [faces], [cam], n_pts=n_pts, corr_radius=0.05)
    assert tuple(pts_traj.shape) == (n_pts, T, 3) and pts_traj.dtype == torch.float64 and tuple(vismask.shape) == (V, T) and vismask.dtype == torch.uint8
    assert v2p.dtype == p2v.dtype == torch.int64 and v2p.shape[1] == p2v.shape[1] == 3 and len(v2p) > 20 and len(p2v) > 20
    for t in range(T):
        a, b = v2p[v2p[:, 2] == t], p2v[p2v[:, 2] == t]
        assert len(a) > 0 and int(a[:, 0].max()) < V and int(a[:, 1].max()) < n_pts and int(b[:, 0].max()) < n_pts and int(b[:, 1].max()) < V
        assert int(a.min()) >= 0 and int(b.min()) >= 0 and bool(vismask[a[:, 0], t].all()) and bool(vismask[b[:, 1], t].all())
    # tracking.deform_batch: the frame's points as DeformNet's input
    edges = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).T
    d = tracking.deform_batch([host(traj[:, 0])], [host(pts_traj[:, 1])], [edges], [edges])
    assert tuple(d.pts.shape) == (n_pts, 3) and d.pts.dtype == torch.float32 and tuple(d.vtx.shape) == (V, 3) and d.pts.is_cuda
    assert tuple(d.pts_batch.shape) == (n_pts,) and d.num_graphs == 1
    # losses.infoNCE: one pair per frame
    gen = torch.Generator().manual_seed(4)
    vf = torch.nn.functional.normalize(torch.randn(V * T, 64, generator=gen), dim=1).cuda()
    pf = torch.nn.functional.normalize(torch.randn(n_pts * T, 64, generator=gen), dim=1).cuda()
    frame_of = lambda n: torch.arange(T).repeat_interleave(n).cuda()
    loss = losses.infoNCE(vf, pf, v2p[:, :2], p2v[:, :2], frame_of(V), frame_of(n_pts), v2p[:, 2].contiguous(), p2v[:, 2].contiguous(), 0.07, num_graphs=T)
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    # playback.trajectory_errors with the scan's mask: a perfect prediction has no error, over all vertices and over the visible ones
    (full, visible), = playback.trajectory_errors([traj], [traj], [vismask])
    assert bool((full == 0).all()) and bool((visible == 0).all()) and bool(vismask.any(dim=0).all())
