"""CPU: the host logic of ``morig_amd.meshprep.simplify`` on an emulated op layer (tests/simplify_emulate.py through
``runtime._test_ops``): the bisection with a resolution per mesh at one host read per step, the launch groups under the 21-bit limit, the
pass-through, the list shapes, the error texts; ``rigging.occluders`` and ``rigging.draw_subsamples``; and ``prepare_mesh`` making, without
``simplify_to``, exactly the calls it made before the argument existed."""
import numpy as np
import pytest
import torch

import meshprep_oracle as mo
import simplify_emulate as se
import simplify_oracle as so
from morig_amd import meshprep, rigging, runtime


@pytest.fixture()
def ops():
    emu = se.SimplifyOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def same(got, want):
    """one mesh's result against the oracle's dict: discrete results equal, positions to a few ulps of the cell size (np.linalg.solve
    on both sides, the sums in the same order)"""
    v, f, m, r = got
    assert v.dtype == torch.float64 and f.dtype == torch.int64 and m.dtype == torch.int64 and isinstance(r, int)
    assert r == want["resolution"] and np.array_equal(m.numpy(), want["vertex_map"]) and np.array_equal(f.numpy(), want["faces"])
    assert tuple(v.shape) == want["verts"].shape and np.array_equal(v.numpy(), want["verts"])


TORUS = mo.torus(12)                                                              # 144 vertices, 288 faces
SPHERE = mo.uv_sphere(12, 8)                                                      # 86 vertices, 168 faces
CUBE = mo.box([0.0] * 3, [1.0, 2.0, 3.0])


def test_bisection_runs_every_mesh_at_its_own_resolution_in_one_launch_per_step(ops):
    meshes = [TORUS, CUBE, SPHERE]
    out, info = meshprep.simplify([m[0] for m in meshes], [m[1] for m in meshes], target_faces=60, return_info=True)
    want = [so.simplify(v, f, 60) for v, f in meshes]
    for g, w in zip(out, want):
        same(g, w)
    assert out[1][3] == 0 and info[1] == [] and torch.equal(out[1][2], torch.arange(8))              # 12 faces: passed through
    assert info[0] == want[0]["trace"] and info[2] == want[2]["trace"] and len(info[0]) == 11       # n(1024), then ten halvings
    for (v, f), w in zip(meshes, want):                                                              # the postconditions
        r = w["resolution"]
        if r:
            assert len(w["faces"]) <= 60 and (r == so.MAX_RES or so.n_faces(v, f, r + 1) > 60)
    # two meshes per launch, every step one launch, the two resolutions differ along the way
    assert set(ops.launch_meshes) == {2} and any(r[0] != r[1] for r in ops.launch_res)
    assert ops.calls.count("simplify_cell_keys") in (11, 12) and ops.calls.count("simplify_quadrics") == 1 and ops.calls.count("mesh_bbox") == 1


def test_given_resolutions_mix_with_targets_and_override_the_pass_through(ops):
    meshes = [TORUS, CUBE, SPHERE]
    out = meshprep.simplify([m[0] for m in meshes], [m[1] for m in meshes], target_faces=100, resolution=[3, 2, None])
    same(out[0], so.simplify(*TORUS, resolution=3))
    same(out[1], so.simplify(*CUBE, resolution=2))                                                   # 12 faces, yet clustered: r was given
    same(out[2], so.simplify(*SPHERE, target_faces=100))
    one, = meshprep.simplify([TORUS[0]], [TORUS[1]], resolution=1)
    assert tuple(one[0].shape) == (1, 3) and tuple(one[1].shape) == (0, 3) and one[1].dtype == torch.int64 and not one[2].any()
    assert meshprep.simplify([], []) == [] and meshprep.simplify([], [], return_info=True) == ([], [])


def test_launch_groups_stay_under_the_index_limit(ops, monkeypatch):
    meshes = [TORUS, SPHERE, TORUS, SPHERE]
    whole = meshprep.simplify([m[0] for m in meshes], [m[1] for m in meshes], target_faces=50)
    assert set(ops.launch_meshes) == {4}
    ops.launch_meshes.clear()
    monkeypatch.setattr(meshprep, "SIMPLIFY_MAX_INDEX", 300)                                         # 144 + 86 fit, a third mesh does not
    split = meshprep.simplify([m[0] for m in meshes], [m[1] for m in meshes], target_faces=50)
    assert set(ops.launch_meshes) == {2} and ops.calls.count("simplify_quadrics") == 3
    for a, b in zip(whole, split):
        assert a[3] == b[3] and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    monkeypatch.setattr(meshprep, "SIMPLIFY_MAX_INDEX", 100)
    with pytest.raises(ValueError, match=r"mesh 0 has 144 vertices: output vertices are numbered in 21 bits"):
        meshprep.simplify([TORUS[0]], [TORUS[1]], target_faces=50)
    same(meshprep.simplify([TORUS[0]], [TORUS[1]], target_faces=288)[0], so.simplify(*TORUS, 288))   # passed through: no limit applies


def test_error_texts(ops):
    v, f = TORUS
    with pytest.raises(ValueError, match="resolution 0: supported are 1 .. 1024"):
        meshprep.simplify([v], [f], resolution=0)
    with pytest.raises(ValueError, match="resolution 1025"):
        meshprep.simplify([v], [f], resolution=[1025])
    with pytest.raises(ValueError, match="one resolution per mesh"):
        meshprep.simplify([v], [f], resolution=[2, 3])
    with pytest.raises(ValueError, match="target_faces"):
        meshprep.simplify([v], [f], target_faces=-1)
    with pytest.raises(ValueError, match="simplify: a face names a vertex outside its mesh"):
        meshprep.simplify([v], [f + 1], target_faces=10)
    with pytest.raises(ValueError, match="simplify: faces are integer"):
        meshprep.simplify([v], [f.astype(np.float64)], target_faces=10)
    with pytest.raises(ValueError, match="simplify: one faces array per mesh"):
        meshprep.simplify([v, v], [f], target_faces=10)
    with pytest.raises(ValueError, match="has no extent"):
        meshprep.simplify([np.zeros((3, 3))], [np.array([[0, 1, 2]])], resolution=2)
    with pytest.raises(ValueError, match="not finite"):
        meshprep.simplify([np.array([[0.0, 0, 0], [1, 0, 0], [np.inf, 1, 0]])], [np.array([[0, 1, 2]])], resolution=2)
    assert "simplify_cell_keys" not in ops.calls


def test_occluders_and_draw_subsamples(ops):
    occ = rigging.occluders([TORUS[0], CUBE[0]], [TORUS[1], CUBE[1]], target_faces=80)
    assert len(occ) == 2 and all(len(o) == 2 for o in occ)
    want = so.simplify(*TORUS, 80)
    assert np.array_equal(occ[0][0].numpy(), want["verts"]) and np.array_equal(occ[0][1].numpy(), want["faces"])
    assert np.array_equal(occ[1][0].numpy(), CUBE[0]) and np.array_equal(occ[1][1].numpy(), CUBE[1])   # its own occluder
    state = np.random.get_state()[1].copy()
    ids = rigging.draw_subsamples(4000, 7)
    assert np.array_equal(np.random.get_state()[1], state)                                            # the global generator is left alone
    np.random.seed(7)
    assert np.array_equal(ids, np.random.choice(4000, 1500, replace=False)) and ids.shape == (1500,)
    np.random.seed(3)
    assert np.array_equal(rigging.draw_subsamples(900, 3), np.random.choice(900, 900, replace=False))
    assert np.array_equal(rigging.draw_subsamples(50, 1, n=20), np.random.RandomState(1).choice(50, 20, replace=False))


def test_prepare_mesh_without_simplify_to_makes_the_calls_it_made(monkeypatch):
    from morig_amd import geodesic, graph_build
    calls = []

    def record(name, result):
        def f(*a, **k):
            calls.append((name, [len(x) if isinstance(x, (list, tuple)) else x for x in a], sorted(k)))
            return result(*a, **k)
        return f

    nv = [8, 8]
    monkeypatch.setattr(meshprep, "normalize", record("normalize", lambda vs: [(torch.zeros(n, 3, dtype=torch.float64), np.zeros(3), 1.0) for n in nv]))
    monkeypatch.setattr(meshprep, "tpl_edges", record("tpl_edges", lambda fs, n, self_loops: [torch.zeros(2, 0, dtype=torch.int64)] * 2))
    monkeypatch.setattr(meshprep, "sample_surface", record("sample_surface", lambda vs, fs, **k: ([torch.zeros(4, 3)] * 2, [torch.zeros(4, 3)] * 2)))
    monkeypatch.setattr(meshprep, "voxelize", record("voxelize", lambda vs, fs, dims: ["vox"] * 2))
    monkeypatch.setattr(meshprep, "simplify", record("simplify", lambda vs, fs, target_faces: [
        (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(8, dtype=torch.int64), 2)] * 2))
    monkeypatch.setattr(geodesic, "surface_geodesic_batched", record("surface_geodesic", lambda vs, p, n: [torch.zeros(v.shape[0], v.shape[0]) for v in vs]))
    monkeypatch.setattr(graph_build, "get_geo_edges_from_distance", record("geo_edges", lambda d, *a: torch.zeros(2, 0, dtype=torch.int64)))
    v, f = CUBE
    out = meshprep.prepare_mesh([v, v], [f, f])
    assert [c[0] for c in calls] == ["normalize", "tpl_edges", "sample_surface", "surface_geodesic", "geo_edges", "geo_edges", "voxelize"]
    assert sorted(out[0]) == ["geo_edge_index", "normals", "pivot", "samples", "scale", "tpl_edge_index", "verts", "vox"]
    assert calls[1][1][1] == 2 and out[0]["verts"].shape[0] == 8
    calls.clear()
    out = meshprep.prepare_mesh(v, f, simplify_to=6)
    assert [c[0] for c in calls][:3] == ["normalize", "simplify", "tpl_edges"] and calls[1][2] == ["target_faces"]
    assert sorted(out) == ["faces", "geo_edge_index", "normals", "pivot", "samples", "scale", "tpl_edge_index", "vertex_map", "verts", "vox"]
    assert out["verts"].shape[0] == 4 and out["faces"].shape == (2, 3) and out["vertex_map"].shape == (8,)
