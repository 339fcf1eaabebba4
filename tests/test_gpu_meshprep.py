"""GPU: morig_amd/meshprep.py (csrc/meshprep.hip) against tests/meshprep_oracle.py -- the 1-ring edges, the reference's normalize bit for
bit, the voxeliser on on-grid scenes (whole grids, no voxel excused: every quantity of the separating-axis test is exact there, and this
is where the touching rule is tested) at every size class of the bitset rows, on generated scenes, in ragged batches, the sampler, and
prepare_mesh's results going through the stages that consume them."""
import json
import os

import numpy as np
import pytest
import torch

import meshprep_oracle as mo
from morig_amd import formats, joints, meshprep, models, skeleton, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIMS = (1, 31, 32, 33, 64, 65, 88, 96)        # one voxel; either side of the 32- and 64-bit word boundaries of a row; the reference's 88; the largest
_cache = {}


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), {k: z[k] for k in z.files if k != "meta"}


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------- edges
def edge_cases():
    fan = np.array([[0, 1 + k, 1 + (k + 1) % 300] for k in range(300)])
    _, tf = mo.torus(24)
    return {"one_triangle": (np.array([[0, 1, 2]]), 3),
            "repeated_index": (np.array([[4, 4, 2]]), 6),
            "duplicate_faces": (np.array([[0, 1, 2], [2, 0, 1], [0, 1, 2], [1, 2, 3]]), 4),
            "isolated_vertex": (np.array([[0, 1, 2], [2, 3, 5]]), 7),
            "fan_300": (fan, 301),
            "cube": (mo.BOX_FACES, 8),
            "torus": (tf, 576),
            "no_faces": (np.zeros((0, 3), dtype=np.int64), 5)}


@pytest.mark.parametrize("name", list(edge_cases()))
def test_tpl_edges_equal_the_oracle(name):
    faces, n = edge_cases()[name]
    got, = meshprep.tpl_edges([faces], [n])
    want = mo.tpl_edges(faces, n)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == want.shape and np.array_equal(host(got), want)
    loops, = meshprep.tpl_edges([torch.as_tensor(faces).int()], [n], self_loops=True)
    assert torch.equal(loops, formats._with_self_loops(torch.from_numpy(want), n).to(loops.device))
    if name == "fan_300":
        assert int((got[0] == 0).sum()) == 300


def test_tpl_edges_of_a_ragged_batch_equal_the_single_runs():
    c = edge_cases()
    names = ["one_triangle", "cube", "no_faces", "torus", "fan_300"]                   # 1, 12, 0, 1152, 300 faces
    batch = meshprep.tpl_edges([c[n][0] for n in names], [c[n][1] for n in names])
    for n, e in zip(names, batch):
        alone, = meshprep.tpl_edges([c[n][0]], [c[n][1]])
        assert torch.equal(e, alone) and np.array_equal(host(e), mo.tpl_edges(*c[n])), n
    with pytest.raises(ValueError, match="outside its mesh"):
        meshprep.tpl_edges([np.array([[0, 1, 3]])], [3])


def test_tpl_edges_equal_the_reference_sets():
    _, a = golden("meshprep_tpl_edges")
    for name in ("cube", "torus", "odd"):
        got, = meshprep.tpl_edges([a[f"{name}_faces"]], [int(a[f"{name}_n"])])
        assert {(int(v), int(w)) for v, w in host(got).T} == {(int(v), int(w)) for v, w in a[f"{name}_edges"]}
        assert np.array_equal(host(got)[0], a[f"{name}_edges"][:, 0])


# ------------------------------------------------------------------------------------------------------------------------- normalize
def test_normalize_is_the_reference_bit_for_bit():
    _, a = golden("meshprep_normalize")
    res = meshprep.normalize([a["in0"], a["in1"]])
    for k, (v, pivot, scale) in enumerate(res):
        assert v.is_cuda and v.dtype == torch.float64
        assert np.array_equal(host(v), a[f"out{k}"]) and np.array_equal(pivot, a[f"pivot{k}"]) and scale == float(a[f"scale{k}"])
        alone, = meshprep.normalize([a[f"in{k}"]])
        assert torch.equal(alone[0], v) and np.array_equal(alone[1], pivot) and alone[2] == scale
    (v, pivot, scale), _ = meshprep.normalize([a["in0"], a["in1"]], pivot=[a["given_pivot"], None], scale=[float(a["given_scale"]), None])
    assert np.array_equal(host(v), a["out_given"]) and np.array_equal(pivot, a["given_pivot"]) and scale == float(a["given_scale"])
    ragged = [a["in0"], a["in1"][:257], a["in0"][:3], a["in1"][:2]]
    for got, src in zip(meshprep.normalize(ragged), ragged):
        assert np.array_equal(host(got[0]), mo.normalize(src)[0])
    with pytest.raises(ValueError, match="no extent"):
        meshprep.normalize([a["in1"][:1]])


# ------------------------------------------------------------------------------------------------------------------------- voxels, on-grid
def on_grid(dims):
    """the scenes of one size, the oracle's grids (computed once) and the product's, all scenes in one batch"""
    if dims not in _cache:
        scenes = mo.on_grid_scenes(dims)
        want = {n: mo.voxelize(v, f, dims) for n, (v, f) in scenes.items()}
        got, info = meshprep.voxelize([v for v, _ in scenes.values()], [f for _, f in scenes.values()], dims=dims, return_info=True)
        _cache[dims] = (scenes, want, dict(zip(scenes, got)), dict(zip(scenes, info)))
    return _cache[dims]


@pytest.mark.parametrize("dims", DIMS)
def test_voxelize_on_grid_scenes_equals_the_oracle_voxel_for_voxel(dims):
    scenes, want, got, info = on_grid(dims)
    assert len(scenes) == (3 if dims == 1 else 12)
    for name in scenes:
        g, w = got[name], want[name]
        assert isinstance(g, formats.Voxels) and g.data.dtype == bool and g.data.shape == (dims,) * 3 and g.dims == [dims] * 3
        assert g.translate == [0.0, 0.0, 0.0] and g.scale == float(dims)
        wrong = int((g.data != w["data"]).sum())
        assert wrong == 0, (dims, name, wrong, int(w["data"].sum()))
        assert info[name][0] == 0
    assert got["grid_cube"].data.all()
    if dims >= 16:
        assert np.array_equal(got["nested_boxes"].data, got["closed_box"].data)          # the cavity is filled
        assert np.array_equal(got["open_box"].data, want["open_box"]["surface"])         # the leak: shell only
        layers = np.nonzero(got["plate_in_a_grid_plane"].data.any(axis=(0, 1)))[0]
        assert len(layers) == 2                                                          # a face in a grid plane sets both neighbours
        assert got["closed_box"].data.sum() > want["closed_box"]["surface"].sum()
    if dims >= 31:
        print(f"dims {dims}: the corridor took {info['corridor'][1]} sweeps")
        assert info["corridor"][1] > 100
        free = ~want["corridor"]["surface"]
        assert free[:, :, dims - 1].any() and (dims < 33 or (free[:, :, 31] & free[:, :, 32]).any())
        assert dims < 65 or (free[:, :, 63] & free[:, :, 64]).any()


# ------------------------------------------------------------------------------------------------------------------------- voxels, generated
def generated(name, attempt):
    rng = np.random.default_rng([0x766F78, attempt])
    if name == "sphere":
        v, f = mo.uv_sphere(32, 16, radius=1.0)
        return v @ mo.rotation(rng).T + rng.normal(size=3), f
    if name == "torus":
        v, f = mo.torus(24)
        return v @ mo.rotation(rng).T + rng.normal(size=3), f
    centres = rng.uniform(0, 1, size=(200, 1, 3))
    v = (centres + rng.normal(size=(200, 3, 3)) * 0.04).reshape(-1, 3)
    return v, np.arange(600).reshape(200, 3)


@pytest.mark.parametrize("name", ["sphere", "torus", "random_triangles"])
def test_voxelize_generated_scenes_equal_the_oracle_outside_its_margin(name):
    """A voxel whose closest separating-axis margin in the oracle is under 1e-9 grid units may be left out, at most 0.1 % of the
    scene's surface voxels; the scene is drawn again until the oracle alone is under that cap. Expected: none left out, bit-equal."""
    dims = 88
    for attempt in range(20):
        v, f = generated(name, attempt)
        want = mo.voxelize(v, f, dims)
        if want["near"].sum() <= 1e-3 * want["surface"].sum():
            break
    else:
        raise AssertionError("no draw keeps the oracle's own near-margin voxels under the cap")
    got, = meshprep.voxelize([v], [f], dims=dims)
    assert got.translate == want["translate"].tolist() and got.scale == float(want["scale"])
    keep = ~want["near"]
    wrong = int((got.data != want["data"])[keep].sum())
    print(f"{name}: {int(want['surface'].sum())} surface voxels, {int(want['data'].sum())} solid, {int(want['near'].sum())} within the margin "
          f"(draw {attempt}), {wrong} differ outside it, {int((got.data != want['data']).sum())} differ in all")
    assert wrong == 0
    if name != "random_triangles":
        assert want["data"].sum() > 2 * want["surface"].sum()


def test_a_ragged_batch_in_two_orders_equals_the_single_runs():
    dims = 33
    scenes = mo.on_grid_scenes(dims)
    sv, sf = generated("sphere", 0)
    meshes = [scenes["corridor"], (sv, sf), scenes["triangle_in_one_voxel"], scenes["nested_boxes"], generated("random_triangles", 1)]
    alone = [meshprep.voxelize([v], [f], dims=dims)[0] for v, f in meshes]
    for order in ([0, 1, 2, 3, 4], [3, 2, 4, 0, 1]):
        batch = meshprep.voxelize([meshes[i][0] for i in order], [torch.as_tensor(meshes[i][1]) for i in order], dims=dims)
        for i, g in zip(order, batch):
            assert np.array_equal(g.data, alone[i].data) and g.translate == alone[i].translate and g.scale == alone[i].scale
    assert np.array_equal(alone[0].data, mo.voxelize(*meshes[0], dims)["data"])


# ------------------------------------------------------------------------------------------------------------------------- samples
def test_sample_surface_equals_the_oracle_and_lies_on_its_triangles():
    """Integers (the triangle of every candidate, the picks of the thinning) are compared exactly; coordinates within 1e-12, the bound the
    reconstruction below has: the inputs are O(1) and every operation is float64 in the oracle's order."""
    rng = np.random.default_rng(0x73616D)
    tv, tf = mo.torus(24)
    tv = mo.normalize(tv @ mo.rotation(rng).T)[0]
    cv, cf = mo.box([0, 0, 0], [1, 2, 3])
    cf = np.concatenate([cf, [[0, 0, 1]]])                                             # a zero-area face is never chosen
    meshes, n, over = [(tv, tf), (cv, cf)], 200, 5
    pts, nrm, tri = meshprep.sample_surface([m[0] for m in meshes], [m[1] for m in meshes], n_samples=n, oversample=over, seed=[7, 8], return_faces=True)
    again = meshprep.sample_surface([m[0] for m in meshes], [m[1] for m in meshes], n_samples=n, oversample=over, seed=[7, 8])
    for b, (v, f) in enumerate(meshes):
        assert torch.equal(pts[b], again[0][b]) and torch.equal(nrm[b], again[1][b])   # two runs, the same bits
        wp, wn, wt, _ = mo.sample_surface(v, f, n, over, 7 + b)
        p, q, t = host(pts[b]), host(nrm[b]), host(tri[b])
        assert p.shape == (n, 3) and p.dtype == np.float64 and np.array_equal(t, wt)
        assert np.abs(p - wp).max() <= 1e-12 and np.abs(q - wn).max() <= 1e-12
        A, B, C = v[f[t, 0]], v[f[t, 1]], v[f[t, 2]]
        face_n = np.cross(B - A, C - A)
        face_n /= np.linalg.norm(face_n, axis=1, keepdims=True)
        assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 1e-12 and np.abs(q - face_n).max() <= 1e-12
        # barycentric weights of p in its triangle (least squares in the triangle's plane), then the point they give
        w12 = np.stack([np.linalg.lstsq(np.stack([B[i] - A[i], C[i] - A[i]], 1), p[i] - A[i], rcond=None)[0] for i in range(n)])
        w = np.concatenate([1 - w12.sum(1, keepdims=True), w12], 1)
        back = w[:, :1] * A + w[:, 1:2] * B + w[:, 2:] * C
        assert np.abs(back - p).max() <= 1e-12 and w.min() >= -1e-12
        alone = meshprep.sample_surface([v], [f], n_samples=n, oversample=over, seed=7 + b)
        assert torch.equal(alone[0][0], pts[b]) and torch.equal(alone[1][0], nrm[b])
    assert not (host(tri[1]) == 12).any()
    with pytest.raises(ValueError, match="no surface area"):
        meshprep.sample_surface([cv], [np.array([[0, 0, 1], [2, 2, 2]])], n_samples=10)


# ------------------------------------------------------------------------------------------------------------------------- all of it
def prepared():
    if "prep" not in _cache:
        mesh = synth.make_mesh(5, n_side=24, with_skin=False, geo="none")
        _, faces = mo.torus(24)
        out = meshprep.prepare_mesh(mesh.pos.numpy().astype(np.float64) * 2.5 + [1.0, -2.0, 0.5], faces, radius=0.15, max_nn=8, seed=3, n_samples=600)
        _cache["prep"] = (mesh, faces, out)
    return _cache["prep"]


def test_prepare_mesh_feeds_the_voxel_stages():
    mesh, faces, out = prepared()
    V = mesh.pos.shape[0]
    assert out["verts"].shape == (V, 3) and out["samples"].shape == out["normals"].shape == (600, 3)
    want_v, pivot, scale = mo.normalize(mesh.pos.numpy().astype(np.float64) * 2.5 + [1.0, -2.0, 0.5])
    assert np.array_equal(host(out["verts"]), want_v) and np.array_equal(out["pivot"], pivot) and out["scale"] == scale
    vox = out["vox"]
    assert np.array_equal(vox.data, mo.voxelize(want_v, faces, 88)["data"])
    # the centre line of the tube, from the vertex rings' centroids
    ring = host(out["verts"]).reshape(24, 24, 3).mean(axis=1)
    line = torch.from_numpy(np.concatenate([ring, (ring + np.roll(ring, 1, 0)) / 2])).cuda()
    inside, idx = joints.inside_check(line, vox)
    assert inside.shape == line.shape and idx.numel() == len(line)
    outside, _ = joints.inside_check(torch.tensor([[0.0, 0.1, 0.0], [2.0, 2.0, 2.0]], dtype=torch.float64).cuda(), vox)
    assert outside.numel() == 0                                                        # the hole of the torus, and a point off the grid
    data = skeleton.make_data(synth.collate([mesh]), [ring[::4]], [vox])
    assert data.pair_attr.shape == (15, 3) and data.outside_count.shape == (15,)
    assert float(data.pair_attr[0, 1]) > 0.9                                           # the bone between two neighbouring joints stays in the tube


def test_prepare_mesh_edges_run_through_a_network_forward():
    mesh, faces, out = prepared()
    V = mesh.pos.shape[0]
    tpl, geo = out["tpl_edge_index"], out["geo_edge_index"]
    assert np.array_equal(host(tpl), mo.tpl_edges(faces, V, self_loops=True))
    assert geo.shape[0] == 2 and geo.shape[1] > V and int(geo.min()) >= 0 and int(geo.max()) < V
    assert int((geo[0] == geo[1]).sum()) == V and int((geo[0] != geo[1]).sum()) > V    # the datasets' self loops, and real balls
    mesh.pos = out["verts"].float().cpu()
    mesh.tpl_edge_index, mesh.geo_edge_index = tpl.cpu(), geo.cpu()
    batch = synth.collate([mesh]).to("cuda")
    net = synth.load_recipe(models.jointnet_motion(num_keyframes=5, chn_output=3, aggr_method="attn").eval(), 3, mild=True).to("cuda")
    res = net(batch, batch.pred_flow)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(r).all()) for r in res) and res[0].shape[0] == V
