"""CPU: the host logic of morig_amd/scan.py on an emulated op layer (tests/scan_emulate.py through ``runtime._test_ops``): the view tables
and ``view_mesh``, the [V, T, 3] -> per-view layout, the chunking, the ``n_pts`` errors, the status handling and the frame column of the
correspondences."""
import numpy as np
import pytest
import torch

import scan_emulate as se
import scan_oracle as so
from morig_amd import runtime, scan


@pytest.fixture()
def ops():
    emu = se.ScanOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


W, H = 24, 20
CAM_O = scan.Camera.orthographic((0.2, 0.3, 3.0), (0, 0, 0), (0, 1, 0), 1.1, 1.1 * H / W, W, H)
CAM_P = scan.Camera.pinhole((0.4, 0.5, 2.6), (0, 0, 0), (0, 1, 0), 45.0, W + 3, H - 2)


def small_torus(seed=5):
    return so.torus(n=8, seed=seed)


def frames(verts, T):
    """[V, T, 3]: the mesh turning about y"""
    out = []
    for t in range(T):
        a = 0.4 * t
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        out.append(verts @ R.T)
    return np.stack(out, 1)


def same(a, b):
    a, b = (x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def test_render_views_share_the_face_table_through_view_mesh(ops):
    v0, f0 = small_torus()
    v1, f1 = so.random_triangles(12)
    traj = frames(v0, 2)
    out = scan.render([traj[:, 0], v1, traj[:, 1]], [f0, f1], [CAM_O, CAM_P, CAM_P], view_mesh=[0, 1, 0])
    assert ops.calls == ["scan_raster", "scan_resolve"] and ops.raster_views == [3]
    for (depth, face, point), (v, f, cam) in zip(out, [(traj[:, 0], f0, CAM_O), (v1, f1, CAM_P), (traj[:, 1], f0, CAM_P)]):
        want = so.render(v, f, cam.row(), cam.kind, cam.width, cam.height)
        assert tuple(depth.shape) == (cam.height, cam.width) and face.dtype == torch.int32 and tuple(point.shape) == (cam.height, cam.width, 3)
        assert same(depth, want["depth"]) and same(face, want["face"]) and same(point, want["point"])
        assert (face >= 0).any() and (face < 0).any()
    assert scan.render([], [], []) == []
    with pytest.raises(ValueError, match="view_mesh"):
        scan.render([v0], [f0], [CAM_O], view_mesh=[1])
    with pytest.raises(ValueError, match="one Camera per view"):
        scan.render([v0, v0], [f0], [CAM_O], view_mesh=[0, 0])
    with pytest.raises(ValueError, match="an earlier view of mesh 0"):
        scan.render([v0, v0[:-1]], [np.zeros((0, 3), dtype=np.int64)], [CAM_O, CAM_O], view_mesh=[0, 0])


def test_scan_meshes_equals_the_oracle_and_thins_by_fps(ops):
    v0, f0 = small_torus()
    for n_pts in (None, 40):
        got, = scan.scan_meshes([v0], [f0], [CAM_O], n_pts=n_pts, corr_radius=0.08)
        img = so.render(v0, f0, CAM_O.row(), CAM_O.kind, W, H)
        vis, _ = so.visibility(v0, f0, CAM_O.row(), CAM_O.kind, W, H, 1e-4)
        want = so.scan_from_images(v0, img["face"], img["point"], vis, n_pts, 0.08)
        assert same(got.vismask, vis) and got.vismask.dtype == torch.uint8
        for name in ("pts", "pixel", "face", "corr_v2p", "corr_p2v"):
            assert same(getattr(got, name), want[name]), name
        assert len(want["corr_v2p"]) > 5 and len(want["corr_p2v"]) > 5 and 0 < vis.sum() < len(vis)
        assert np.all(np.diff(want["corr_v2p"][:, 0]) > 0) and np.all(np.diff(want["corr_p2v"][:, 0]) > 0)
        assert vis[want["corr_v2p"][:, 0]].all() and vis[want["corr_p2v"][:, 1]].all()
        assert ("fps" in ops.calls) == (n_pts is not None)


def test_trajectory_layout_and_the_frame_column(ops):
    v0, f0 = small_torus()
    v1, f1 = small_torus(seed=8)
    T, n_pts = 3, 32
    traj = [frames(v0, T), frames(v1[:50], T)]
    f1 = f1[(f1 < 50).all(axis=1)]
    out = scan.scan_trajectory(traj, [f0, f1], [CAM_O, [CAM_O, CAM_P, CAM_O]], n_pts=n_pts, corr_radius=0.1)
    assert ops.raster_views == [2 * T]
    for m, (pts_traj, vismask, v2p, p2v) in enumerate(out):
        V = traj[m].shape[0]
        assert tuple(pts_traj.shape) == (n_pts, T, 3) and pts_traj.dtype == torch.float64 and tuple(vismask.shape) == (V, T)
        assert vismask.dtype == torch.uint8 and v2p.dtype == p2v.dtype == torch.int64 and v2p.shape[1] == p2v.shape[1] == 3
        assert np.all(np.diff(v2p[:, 2].numpy()) >= 0) and set(v2p[:, 2].tolist()) <= set(range(T)) and len(v2p) > 0 and len(p2v) > 0
        for t in range(T):
            cam = CAM_O if m == 0 else [CAM_O, CAM_P, CAM_O][t]
            one, = scan.scan_meshes([traj[m][:, t]], [[f0, f1][m]], [cam], n_pts=n_pts, corr_radius=0.1)
            assert same(pts_traj[:, t], one.pts) and same(vismask[:, t], one.vismask)
            assert same(v2p[v2p[:, 2] == t][:, :2], one.corr_v2p) and same(p2v[p2v[:, 2] == t][:, :2], one.corr_p2v)
            assert one.corr_v2p[:, 0].max() < V and one.corr_v2p[:, 1].max() < n_pts and one.corr_p2v[:, 0].max() < n_pts
    with pytest.raises(ValueError, match="n_pts is required"):
        scan.scan_trajectory(traj, [f0, f1], [CAM_O, CAM_O], n_pts=None)
    with pytest.raises(ValueError, match="3 frames and 2 cameras"):
        scan.scan_trajectory(traj, [f0, f1], [CAM_O, [CAM_O, CAM_P]], n_pts=8)
    with pytest.raises(ValueError, match=r"\[V, T, 3\]"):
        scan.scan_trajectory([traj[0][:, 0]], [f0], [CAM_O], n_pts=8)


def test_a_budget_that_forces_chunks_gives_the_result_of_one_chunk(ops):
    v0, f0 = small_torus()
    traj = [frames(v0, 5)]
    whole = scan.scan_trajectory(traj, [f0], [CAM_O], n_pts=24, corr_radius=0.1)
    assert ops.raster_views == [5]
    ops.raster_views.clear()
    parts = scan.scan_trajectory(traj, [f0], [CAM_O], n_pts=24, corr_radius=0.1, key_budget=2 * 8 * W * H)
    assert ops.raster_views == [2, 2, 1]
    for a, b in zip(whole[0], parts[0]):
        assert same(a, b)
    ops.raster_views.clear()
    scan.render([traj[0][:, t] for t in range(3)], [f0], [CAM_O] * 3, view_mesh=[0, 0, 0], key_budget=1)      # a view above the budget goes alone
    assert ops.raster_views == [1, 1, 1]


def test_n_pts_errors_name_the_view(ops):
    v0, f0 = small_torus()
    hits = int((so.render(v0 * 0.5, f0, CAM_O.row(), CAM_O.kind, W, H)["face"] >= 0).sum())
    assert 0 < hits < int((so.render(v0, f0, CAM_O.row(), CAM_O.kind, W, H)["face"] >= 0).sum())
    with pytest.raises(ValueError, match=f"view 1 has {hits} hits, fewer than n_pts = {hits + 1}"):              # view 1 is in the second chunk
        scan.scan_meshes([v0, v0 * 0.5], [f0], [CAM_O, CAM_O], n_pts=hits + 1, view_mesh=[0, 0], key_budget=1)
    cover = scan.Camera.orthographic(**so.on_grid_camera(256, 256))
    cv, cf = so.on_grid_scenes(256, 256)["cover"]
    with pytest.raises(ValueError, match="view 0 has 65536 hits: thinning to n_pts takes at most 32768"):
        scan.scan_meshes([cv], [cf], [cover], n_pts=100)
    assert scan.scan_meshes([cv], [cf], [cover])[0].pts.shape[0] == 65536
    for bad in (0, 32769):
        with pytest.raises(ValueError, match="n_pts"):
            scan.scan_meshes([v0], [f0], [CAM_O], n_pts=bad)
    with pytest.raises(ValueError, match="corr_radius"):
        scan.scan_meshes([v0], [f0], [CAM_O], corr_radius=-1.0)


def test_status_of_a_bad_face_is_a_value_error(ops):
    v0, f0 = small_torus()
    bad = f0.copy()
    bad[3, 1] = len(v0)
    for call in (lambda: scan.render([v0], [bad], [CAM_O]), lambda: scan.scan_meshes([v0], [bad], [CAM_O])):
        with pytest.raises(ValueError, match="a face names a vertex outside its mesh"):
            call()
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="a face names a vertex outside its mesh"):
        scan.render([v0], [bad], [CAM_O])
    with pytest.raises(ValueError, match="integer"):
        scan.render([v0], [f0.astype(np.float64)], [CAM_O])


def test_empty_views_and_views_without_hits(ops):
    v0, f0 = small_torus()
    out = scan.scan_meshes([np.zeros((0, 3)), v0 + [50.0, 0, 0], v0], [np.zeros((0, 3), dtype=np.int64), f0], [CAM_O, CAM_O, CAM_P], view_mesh=[0, 1, 1])
    assert out[0].pts.shape == (0, 3) and out[0].vismask.shape == (0,) and out[0].corr_v2p.shape == (0, 2)
    assert out[1].pts.shape == (0, 3) and not out[1].vismask.any() and out[1].corr_p2v.shape == (0, 2)
    assert out[2].pts.shape[0] > 0 and out[2].vismask.any()
