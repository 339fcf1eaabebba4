"""CPU: the oracle of the mesh front end (tests/meshprep_oracle.py) held to the reference's own results (tests/golden/meshprep_*.npz, made
by tools/make_meshprep_golden.py) and to two analytic scenes; the binvox and OBJ formats of morig_amd/formats.py; the separating-axis core
csrc/tribox_core.h as the stand-alone program tools/tribox_host_check.cpp, built with the address and undefined-behaviour sanitizers and
run as a program (never loaded into Python), against the oracle's test; the new exports' refusals through the C ABI."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import meshprep_oracle as mo
from morig_amd import abi, formats, meshprep, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), {k: z[k] for k in z.files if k != "meta"}


# ------------------------------------------------------------------------------------------------------------------------- normalize, edges
def test_oracle_normalize_is_the_reference_bit_for_bit():
    _, a = golden("meshprep_normalize")
    for k in range(2):
        v, pivot, scale = mo.normalize(a[f"in{k}"])
        assert np.array_equal(v, a[f"out{k}"]) and np.array_equal(pivot, a[f"pivot{k}"]) and scale == float(a[f"scale{k}"])
    given = (a["in0"] - a["given_pivot"]) * float(a["given_scale"])
    assert np.array_equal(given, a["out_given"])


@pytest.mark.parametrize("name", ["cube", "torus", "odd"])
def test_oracle_edge_set_is_the_reference_set(name):
    _, a = golden("meshprep_tpl_edges")
    n = int(a[f"{name}_n"])
    want = {(int(v), int(w)) for v, w in a[f"{name}_edges"]}
    assert mo.tpl_edge_set(a[f"{name}_faces"], n) == want
    e = mo.tpl_edges(a[f"{name}_faces"], n)
    assert e.shape == (2, len(want)) and e.dtype == np.int64
    keys = e[0] * n + e[1]
    assert (np.diff(keys) > 0).all()                                                   # ascending v, then ascending n
    # the reference lists a vertex's neighbours together and the vertices in ascending order: the grouping is the same
    assert np.array_equal(e[0], a[f"{name}_edges"][:, 0])
    loops = mo.tpl_edges(a[f"{name}_faces"], n, self_loops=True)
    assert np.array_equal(loops[:, len(want):], np.tile(np.arange(n), (2, 1)))
    if name == "odd":
        assert 7 not in e[0] and 7 not in e[1] and (3, 4) in want and (3, 3) not in want


# ------------------------------------------------------------------------------------------------------------------------- formats
@pytest.mark.parametrize("name", ["torus", "crafted"])
def test_binvox_bytes_both_ways(name, tmp_path):
    meta, a = golden("meshprep_binvox")
    dims = [int(d) for d in a[f"{name}_dims"]]
    data = np.unpackbits(a[f"{name}_bits"])[:int(np.prod(dims))].astype(bool).reshape(dims)
    vox = formats.Voxels(data, dims, a[f"{name}_translate"], a[f"{name}_scale"])
    assert vox.dims == dims and isinstance(vox.scale, float) and isinstance(vox.translate, list)
    path = str(tmp_path / "m.binvox")
    formats.write_binvox(vox, path)
    raw = open(path, "rb").read()
    assert raw == a[f"{name}_file"].tobytes()                                          # byte-equal to the reference's write
    if name == "crafted":
        assert meta["crafted_zero_count_pairs"] >= 2                                   # runs of 255 and 510: the reference's count-0 pairs
    with open(path, "wb") as f:
        f.write(a[f"{name}_file"].tobytes())
    back = formats.read_binvox(path)
    want = np.unpackbits(a[f"{name}_read_bits"])[:int(np.prod(dims))].astype(bool).reshape(dims)
    assert back.data.dtype == bool and np.array_equal(back.data, want) and np.array_equal(back.data, data)
    assert back.dims == dims and back.translate == [float(t) for t in a[f"{name}_translate"]] and back.scale == float(a[f"{name}_scale"])
    assert back.data.flags["C_CONTIGUOUS"]


def test_binvox_refuses_what_is_no_binvox_file(tmp_path):
    path = str(tmp_path / "x.binvox")
    with open(path, "wb") as f:
        f.write(b"ply\nformat ascii 1.0\n")
    with pytest.raises(IOError):
        formats.read_binvox(path)
    with pytest.raises(ValueError):
        formats.write_binvox(formats.Voxels(np.zeros((4, 4), dtype=bool), [4, 4, 4], [0, 0, 0], 1.0), path)


OBJ = """# a comment
mtllib ignored.mtl
v 0 0 0
v 1 0 0 0.5 0.5 0.5
vn 0 0 1
vt 0.5 0.5
v 1 1 0
v 0 1 0
o part
g group
f 1 2 3
f 1/1 3/2 4/3
f 1//1 2//1 3//1 4//1
v 0.5 0.5 1.5e0
f -1/4/1 1/1/1 2/2/1
f -5 -4 -3 -2 -1

s off
usemtl none
l 1 2
"""


def test_read_obj_on_a_literal(tmp_path):
    path = str(tmp_path / "m.obj")
    with open(path, "w") as f:
        f.write(OBJ)
    v, faces = formats.read_obj(path)
    assert v.dtype == np.float64 and faces.dtype == np.int64
    assert np.array_equal(v, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.5]])
    assert faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    with open(path, "w") as f:
        f.write("v 0 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="names no vertex"):
        formats.read_obj(path)
    with open(path, "w") as f:
        f.write("# nothing\n")
    v, faces = formats.read_obj(path)
    assert v.shape == (0, 3) and faces.shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------------------- analytic scenes
# A voxel whose centre is more than 2 voxel edges from the analytic surface must equal the analytic inside test: 2 = the cube's half
# diagonal 0.87 plus the largest gap between the polyhedron and the surface it is inscribed in, rounded up. Sphere of 32 x 16 faces,
# r = 44: the chord sagitta r (1 - cos(pi / 32)) = 0.21. Torus of 24 x 24 quads, R + r = 44 voxels: (R + r)(1 - cos(pi / 24)) = 0.38
# around the ring plus r (1 - cos(pi / 24)) = 0.10 around the tube.
BAND = 2.0


def test_sphere_equals_the_analytic_solid_away_from_its_surface():
    v, f = mo.uv_sphere(32, 16, radius=0.5)
    r = mo.voxelize(v, f, 88)
    assert np.allclose(r["translate"], -0.5) and np.isclose(r["scale"], 1.0)
    c = np.arange(88) + 0.5
    dist = np.sqrt((c[:, None, None] - 44) ** 2 + (c[None, :, None] - 44) ** 2 + (c[None, None, :] - 44) ** 2)
    far = np.abs(dist - 44.0) > BAND
    assert far.sum() > 0.8 * 88 ** 3 and np.array_equal(r["data"][far], (dist < 44.0)[far])
    assert r["data"][44, 44, 44] and not r["surface"][44, 44, 44] and not r["data"][0, 0, 0]
    assert not r["near"].all()


def test_torus_equals_the_analytic_solid_away_from_its_surface():
    R0, r0 = 0.35, 0.12
    v, f = mo.torus(24, R0, r0)
    r = mo.voxelize(v, f, 88)
    k = 88 / (2 * (R0 + r0))                                                           # voxels per unit
    assert np.allclose(r["translate"], [-(R0 + r0), 0.0, -(R0 + r0)]) and np.isclose(r["scale"], 2 * (R0 + r0))
    c = (np.arange(88) + 0.5) / k
    x, y, z = c[:, None, None] - (R0 + r0), c[None, :, None], c[None, None, :] - (R0 + r0)
    tube = np.sqrt((np.sqrt(x * x + z * z) - R0) ** 2 + (y - r0) ** 2)                 # distance from the centre circle
    far = np.abs(tube - r0) * k > BAND
    assert far.sum() > 0.8 * 88 ** 3 and np.array_equal(r["data"][far], (tube < r0)[far])
    assert r["data"].sum() > r["surface"].sum() > 0                                    # solid, not a shell


def test_the_touching_rule_and_the_leak_on_small_scenes():
    sc = mo.on_grid_scenes(32)
    plate = mo.voxelize(*sc["plate_in_a_grid_plane"], 32)
    layers = np.nonzero(plate["data"].any(axis=(0, 1)))[0]
    assert layers.tolist() == [15, 16]                                                 # a face in the plane z = 16 sets both neighbours
    closed, opened = mo.voxelize(*sc["closed_box"], 32), mo.voxelize(*sc["open_box"], 32)
    assert closed["data"].sum() > closed["surface"].sum() and np.array_equal(opened["data"], opened["surface"])
    nested = mo.voxelize(*sc["nested_boxes"], 32)
    assert np.array_equal(nested["data"], closed["data"])                              # the cavity is filled
    assert mo.voxelize(*sc["grid_cube"], 32)["data"].all()
    one = mo.voxelize(*sc["triangle_in_one_voxel"], 32)
    assert one["data"].sum() == 1


# ------------------------------------------------------------------------------------------------------------------------- host logic
def test_host_refusals_need_no_device():
    with pytest.raises(ValueError, match="dims 0"):
        meshprep.voxelize([np.zeros((3, 3))], [np.array([[0, 1, 2]])], dims=0)
    with pytest.raises(ValueError, match="dims 97"):
        meshprep.voxelize([np.zeros((3, 3))], [np.array([[0, 1, 2]])], dims=97)
    with pytest.raises(ValueError, match="candidates"):
        meshprep.sample_surface([np.zeros((3, 3))], [np.array([[0, 1, 2]])], n_samples=8000, oversample=5)
    u = meshprep.draw_uniforms(7, 3)
    assert u.shape == (7, 3) and np.array_equal(u, np.random.Generator(np.random.PCG64(3)).random((7, 3)))


def test_new_exports_are_typed_and_refuse_bad_sizes_without_a_device():
    names = ["morig_mesh_bbox", "morig_mesh_affine", "morig_tpl_edge_keys", "morig_tpl_edge_flags", "morig_tpl_edge_compact", "morig_voxel_surface",
             "morig_voxel_fill", "morig_tri_area_cdf", "morig_surface_samples"]
    assert set(names) <= set(native.EXPORTS) and len(abi.STRUCTS) == 8                 # plain parameters: no new argument struct
    lib = native.load_library()
    K = abi.CONSTANTS
    assert K["MORIG_VOXEL_MAX_DIMS"] == meshprep.MAX_DIMS == 96 and K["MORIG_VOXEL_ROW_WORDS"] * 32 >= K["MORIG_VOXEL_MAX_DIMS"]
    for dims in (0, 97, -1):                                                           # refused before anything is launched
        assert lib.morig_voxel_fill(None, 1, dims, None, None, None) == K["MORIG_E_UNSUPPORTED"]
        assert lib.morig_voxel_surface(None, None, 0, None, None, 1, dims, None, None) == K["MORIG_E_UNSUPPORTED"]
    assert lib.morig_voxel_fill(None, 0, 88, None, None, None) == K["MORIG_OK"]
    assert lib.morig_voxel_fill(None, 1, 88, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_mesh_bbox(None, None, 0, None, None) == K["MORIG_OK"] and lib.morig_mesh_bbox(None, None, 2, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_mesh_affine(None, 5, None, 1, None, 7, 1.0, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_tpl_edge_keys(None, -1, None, None, 1, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_tpl_edge_flags(None, 0, None, None) == K["MORIG_OK"] and lib.morig_tpl_edge_flags(None, 4, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_tpl_edge_compact(None, None, None, 4, None, 1, 5, None, None) == K["MORIG_E_INVALID"]       # more edges than keys
    assert lib.morig_surface_samples(None, None, None, None, 1, None, None, None, 3, None, None, None, None) == K["MORIG_E_INVALID"]


# ------------------------------------------------------------------------------------------------------------------------- the host program
def _sat_cases():
    """(triangles [n, 3, 3], voxels [n, 3], exact bool [n]): on-grid triangles against every voxel of their padded box (exact: the
    decisions must agree, touching included), and random ones (a decision within MARGIN of flipping may differ)"""
    tris, voxels, exact = [], [], []
    rng = np.random.default_rng(0x534154)
    on_grid = [np.array([[2.0, 2.0, 2.0], [5.0, 2.0, 2.0], [2.0, 5.0, 2.0]]),                    # in the grid plane z = 2
               np.array([[1.5, 1.0, 3.0], [4.0, 4.5, 3.5], [2.0, 6.0, 1.0]]),
               np.array([[1.0, 1.0, 1.0], [3.0, 3.0, 3.0], [5.0, 5.0, 5.0]]),                    # collinear
               np.array([[2.0, 3.0, 4.0], [2.0, 3.0, 4.0], [4.5, 3.0, 4.0]]),                    # two equal corners
               np.array([[3.0, 3.0, 3.0]] * 3),                                                  # a point on a grid corner: 8 voxels
               np.array([[2.25, 2.25, 2.25], [2.75, 2.25, 2.5], [2.25, 2.75, 2.75]]),            # inside one voxel
               np.array([[0.0, 0.0, 0.0], [8.0, 8.0, 0.0], [0.0, 8.0, 8.0]])]
    for t in on_grid:
        lo, hi = np.floor(t.min(0)).astype(int) - 2, np.ceil(t.max(0)).astype(int) + 1
        idx = np.stack(np.meshgrid(*[np.arange(lo[c], hi[c] + 1) for c in range(3)], indexing="ij"), -1).reshape(-1, 3)
        tris += [t] * len(idx)
        voxels += list(idx)
        exact += [True] * len(idx)
    for _ in range(300):
        t = rng.uniform(0, 12, size=(1, 3)) + rng.normal(size=(3, 3)) * rng.choice([0.2, 1.0, 4.0])
        for _ in range(12):
            tris.append(t)
            voxels.append(np.floor(t[rng.integers(3)] + rng.normal(size=3) * 1.5).astype(int))
            exact.append(False)
    return np.array(tris), np.array(voxels, dtype=np.int32), np.array(exact)


def test_tribox_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "tribox_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "tribox_host_check.cpp"), "-o", exe], check=True)
    tris, voxels, exact = _sat_cases()
    extra_t = np.stack([np.full((3, 3), np.nan), np.full((3, 3), np.inf), np.zeros((3, 3))])     # must not trip the sanitizers
    extra_v = np.array([[0, 0, 0], [1, 1, 1], [-1, -1, -1]], dtype=np.int32)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    n = len(tris) + len(extra_t)
    with open(src, "wb") as f:
        f.write(struct.pack("i", n))
        f.write(np.ascontiguousarray(np.concatenate([tris, extra_t])).tobytes())
        f.write(np.ascontiguousarray(np.concatenate([voxels, extra_v])).tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    got = np.frombuffer(open(dst, "rb").read(), dtype=np.uint8).astype(bool)
    assert got.shape == (n,)
    want, margin = np.zeros(len(tris), dtype=bool), np.zeros(len(tris))
    for q, (t, v) in enumerate(zip(tris, voxels)):
        o, m = mo.sat(t, v, v)
        want[q], margin[q] = o[0, 0, 0], m[0, 0, 0]
    firm = exact | (margin >= mo.MARGIN)
    print(f"tribox_core.h vs the oracle: {len(tris)} decisions, {int(want.sum())} overlaps, {int(exact.sum())} exact, "
          f"{int((~firm).sum())} within {mo.MARGIN} of flipping")
    assert firm.sum() > 0.99 * len(tris) and want[exact].sum() > 100 and (~want[exact]).sum() > 100
    assert np.array_equal(got[:len(tris)][firm], want[firm])
    assert got[len(tris) + 2] and not got[len(tris) + 1]                               # the origin touches voxel (-1, -1, -1); inf overlaps nothing
