"""CPU: the oracle of the mesh simplification (tests/simplify_oracle.py) on answers known by hand and on the properties the rule is meant
to have; the per-cell arithmetic csrc/quadric_core.h as the stand-alone program tools/quadric_host_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a program (never loaded into Python), against the oracle; the new exports' refusals through
the C ABI.

Figures measured here (printed by the tests): the output vertices with every sum taken forwards against every sum taken backwards differ
by at most 1.9e-13 of a cell size h on the position fixtures (1e-15 to 2e-14 h on the unrotated ones, 3e-29 h where every cell holds one
vertex); quadric_host_check (Cholesky) against the oracle (np.linalg.solve), the sums in the same order, by at most 5.4e-14 h on 1 002
cells, 703 of them equal bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import meshprep_oracle as mo
import simplify_oracle as so
from morig_amd import abi, meshprep, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------- by hand
def test_two_triangles_in_one_cell_give_one_vertex_and_no_face():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])
    out = so.simplify(v, [[0, 1, 2], [1, 3, 2]], resolution=1)
    assert out["verts"].shape == (1, 3) and out["faces"].shape == (0, 3) and not out["vertex_map"].any()
    assert np.all(out["verts"] >= 0) and np.all(out["verts"] <= 1)


def test_tetrahedron_at_resolution_two():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    out = so.simplify(v, f, resolution=2)
    assert out["vertex_map"].tolist() == [0, 3, 2, 1]                                  # keys 0, 4, 2, 1: ascending key is vertex 0, 3, 2, 1
    assert out["faces"].tolist() == [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]      # by sorted triple; orientation kept, smallest first
    assert np.array_equal(out["verts"], v[[0, 3, 2, 1]])                               # every plane of a cell passes through its one vertex
    assert out["resolution"] == 2 and out["h"] == 0.5


def test_the_lower_input_face_keeps_its_orientation():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    for first, second in (([1, 2, 3], [1, 3, 2]), ([1, 3, 2], [1, 2, 3]), ([3, 1, 2], [2, 1, 3])):
        out = so.simplify(v, [first, second, second, first], resolution=2)
        m = out["vertex_map"][np.array(first)].tolist()                                # [3, 2, 1] in some rotation
        k = m.index(min(m))
        assert out["faces"].tolist() == [m[k:] + m[:k]]


def test_boundary_rules_on_an_exact_grid():
    r = 4
    pts = np.array([[2.0, 1.5, 4.0], [3.0, 0.0, 0.25], [4.0, 4.0, 1.0], [1.0, 1.0, 1.0], [0.5, 3.5, 2.0]])
    v, f = mo.framed([(pts, np.array([[0, 1, 2], [0, 3, 4]]))], r)
    assert np.array_equal(v / r * r, v)                                                # g is exact: a vertex's coordinates are its grid coordinates
    c, key = so.cells(v, r)
    assert c[:5].tolist() == [[2, 1, 3], [3, 0, 0], [3, 3, 1], [1, 1, 1], [0, 3, 2]]   # on the upper box face: r - 1; on a plane: the upper cell
    assert c[5].tolist() == [0, 0, 0] and c[6].tolist() == [3, 3, 3] and key[0] == (2 * 4 + 1) * 4 + 3
    out = so.simplify(v, f, resolution=r)
    lo, hi = c[np.argsort(key)] * 1.0, c[np.argsort(key)] + 1.0                        # every output vertex inside its closed cell
    assert np.all(out["verts"] >= lo) and np.all(out["verts"] <= hi) and len(out["verts"]) == 7


# ------------------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("name", ["torus", "sphere"])
def test_closed_inputs_keep_every_edge_even_before_the_duplicate_removal(name):
    v, f = mo.torus(64) if name == "torus" else mo.uv_sphere(96, 48)
    v = so.rotated(v, 11)
    assert so.odd_edges(f) == []
    for r in (3, 7, 20, 26, 40):
        vmap, _, _ = so.vertex_map(v, r)
        m, _ = so.surviving(f, vmap)
        assert len(m) > 0 and so.odd_edges(m) == []


def test_the_corner_of_a_subdivided_cube_stays_a_corner():
    v, f = so.subdivided_cube(12)
    out = so.simplify(v, f, resolution=3)
    vmap = out["vertex_map"]
    corner = out["verts"][vmap[np.argmax(v.sum(1))]]                                   # the cell of the vertex (1, 1, 1)
    members = v[vmap == vmap[np.argmax(v.sum(1))]]
    print(f"cube 12 x 12 at r = 3: corner cell vertex {1 - corner} from the corner, its centroid {1 - members.mean(0)}")
    assert np.all(np.abs(corner - 1.0) < 1e-3) and np.all(np.abs(members.mean(0) - 1.0) > 0.1)


@pytest.mark.parametrize("target", [3000, 300, 12])
def test_bisection_postconditions(target):
    v, f = so.rotated(mo.torus(64)[0], 2), mo.torus(64)[1]
    r, trace = so.choose_resolution(v, f, target)
    n = dict(trace)
    assert 1 <= r < so.MAX_RES and so.n_faces(v, f, r) <= target < so.n_faces(v, f, r + 1)
    assert n[so.MAX_RES] > target and len(trace) == 11 and all(1 < m < so.MAX_RES for m, _ in trace[1:])
    out = so.simplify(v, f, target)
    assert out["resolution"] == r and len(out["faces"]) == so.n_faces(v, f, r) and out["vertex_map"].max() + 1 == len(out["verts"])
    print(f"torus(64), target {target}: r = {r}, {len(out['verts'])} vertices, {len(out['faces'])} faces")


def test_resolution_1024_is_taken_when_it_fits_and_small_meshes_pass_through():
    v, f = mo.torus(8)
    assert so.choose_resolution(v, f, 128) == (so.MAX_RES, [(so.MAX_RES, 128)])
    out = so.simplify(v, f, 128)
    assert out["resolution"] == 0 and out["verts"] is not None and np.array_equal(out["verts"], v) and np.array_equal(out["faces"], f)
    assert np.array_equal(out["vertex_map"], np.arange(64))
    out = so.simplify(v, f, 127)
    assert out["resolution"] < so.MAX_RES and len(out["faces"]) <= 127


def test_forward_against_reversed_sums_on_the_position_fixtures():
    worst = 0.0
    for name, v, f, r in so.position_fixtures():
        dev = so.order_deviation(v, f, r)
        print(f"{name}: forwards against backwards {dev:.2e} h")
        worst = max(worst, dev)
    assert worst < so.POSITION_CAP / 16                                                # the device bar, 16 times this figure, stays under its cap


# ------------------------------------------------------------------------------------------------------------------------- the ABI
def test_new_exports_are_typed_and_refuse_bad_sizes_without_a_device():
    names = ["morig_simplify_cell_keys", "morig_simplify_face_keys", "morig_simplify_face_compact", "morig_simplify_quadrics"]
    assert set(names) <= set(native.EXPORTS) and len(abi.STRUCTS) == 8                 # plain parameters: no new argument struct
    lib = native.load_library()
    K = abi.CONSTANTS
    assert K["MORIG_SIMPLIFY_MAX_RES"] == meshprep.SIMPLIFY_MAX_RES == 1024 and K["MORIG_SIMPLIFY_INDEX_BITS"] == 21
    assert K["MORIG_SIMPLIFY_MAX_INDEX"] == meshprep.SIMPLIFY_MAX_INDEX == 1 << 21 and K["MORIG_SIMPLIFY_MAX_RES"] ** 3 == 1 << K["MORIG_SIMPLIFY_MESH_SHIFT"]
    big = K["MORIG_SIMPLIFY_MAX_INDEX"] + 1
    for lo, hi in ((0, 5), (1, 1025), (-3, -1), (6, 5)):                               # refused before anything is launched
        assert lib.morig_simplify_cell_keys(None, 4, None, 1, None, None, lo, hi, None, None) == K["MORIG_E_UNSUPPORTED"]
        assert lib.morig_simplify_quadrics(None, 4, None, None, 0, None, 1, None, None, lo, hi, None, None, None, None, None, 1, None,
                                           None) == K["MORIG_E_UNSUPPORTED"]
    assert lib.morig_simplify_cell_keys(None, big, None, 1, None, None, 1, 8, None, None) == K["MORIG_E_UNSUPPORTED"]        # the 21-bit limit
    assert lib.morig_simplify_face_keys(None, 3, None, None, 1, None, big, 5, None, None, None) == K["MORIG_E_UNSUPPORTED"]
    assert lib.morig_simplify_face_keys(None, 3, None, None, 1, None, 5, big, None, None, None) == K["MORIG_E_UNSUPPORTED"]
    assert lib.morig_simplify_quadrics(None, 4, None, None, 0, None, 1, None, None, 1, 8, None, None, None, None, None, big, None,
                                       None) == K["MORIG_E_UNSUPPORTED"]
    assert lib.morig_simplify_cell_keys(None, -1, None, 1, None, None, 1, 8, None, None) == K["MORIG_E_INVALID"]              # negative counts
    assert lib.morig_simplify_cell_keys(None, 4, None, -1, None, None, 1, 8, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_simplify_face_keys(None, -1, None, None, 1, None, 5, 5, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_simplify_face_compact(None, 3, None, None, 1, None, None, None, None, None, -1, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_simplify_face_compact(None, 3, None, None, 1, None, None, None, None, None, 4, None, None) == K["MORIG_E_INVALID"]   # more faces out than in
    assert lib.morig_simplify_quadrics(None, 4, None, None, 0, None, 1, None, None, 1, 8, None, None, None, None, None, -1, None,
                                       None) == K["MORIG_E_INVALID"]
    assert lib.morig_simplify_cell_keys(None, 4, None, 0, None, None, 1, 8, None, None) == K["MORIG_OK"]                     # zero meshes
    assert lib.morig_simplify_face_keys(None, 3, None, None, 0, None, 5, 5, None, None, None) == K["MORIG_OK"]
    assert lib.morig_simplify_face_compact(None, 3, None, None, 0, None, None, None, None, None, 2, None, None) == K["MORIG_OK"]
    assert lib.morig_simplify_quadrics(None, 4, None, None, 0, None, 0, None, None, 1, 8, None, None, None, None, None, 3, None,
                                       None) == K["MORIG_OK"]
    assert lib.morig_simplify_cell_keys(None, 4, None, 1, None, None, 1, 8, None, None) == K["MORIG_E_INVALID"]              # null pointers
    assert lib.morig_simplify_quadrics(None, 4, None, None, 0, None, 1, None, None, 1, 8, None, None, None, None, None, 3, None,
                                       None) == K["MORIG_E_INVALID"]
    names = [lib.morig_prof_name(k) for k in range(K["MORIG_PROF_KINDS"])]
    assert b"simplify_keys" in names and b"simplify_quadrics" in names


def test_host_refusals_need_no_device():
    v, f = mo.torus(8)
    with pytest.raises(ValueError, match="resolution 1025"):
        meshprep.simplify([v], [f], resolution=1025)
    with pytest.raises(ValueError, match="target_faces"):
        meshprep.simplify([v], [f], target_faces=-2)


# ------------------------------------------------------------------------------------------------------------------------- the host program
def test_quadric_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "quadric_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "quadric_host_check.cpp"), "-o", exe], check=True)
    table, grid, members, corners, want, hs = [], [], [], [], [], []
    for name, v, f, r in so.position_fixtures():
        c = so.cell_lists(v, f, r)
        pos, _, h = so.positions(v, f, r)
        for q in range(len(pos)):
            table.append([len(c["members"][q]), len(c["corners"][q]), *c["coord"][q]])
            grid.append([*c["lo"], h])
            members += c["members"][q]
            corners += [sum(t, []) for t in c["corners"][q]]
        want.append(pos)
        hs += [h] * len(pos)
    # zero-area corners only (trace M = 0: the centroid), and a cell whose sums overflow: neither may trip the sanitizers
    table += [[2, 1, 0, 0, 0], [1, 1, 0, 0, 0]]
    grid += [[0.0, 0.0, 0.0, 1.0]] * 2
    members += [[0.25, 0.5, 0.75], [0.75, 0.5, 0.25], [0.5, 0.5, 0.5]]
    corners += [[0.1] * 9, [0.0, 0.0, 0.0, 1e200, 0.0, 0.0, 0.0, 1e200, 0.0]]
    want, hs = np.concatenate(want), np.array(hs)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("=iqq", len(table), len(members), len(corners)))
        fh.write(np.array(table, dtype=np.int32).tobytes())
        fh.write(np.array(grid, dtype=np.float64).tobytes())
        fh.write(np.array(members, dtype=np.float64).tobytes())
        fh.write(np.array(corners, dtype=np.float64).reshape(-1, 9).tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    got = np.frombuffer(open(dst, "rb").read(), dtype=np.float64).reshape(-1, 3)
    assert got.shape == (len(table), 3) and np.array_equal(got[-2], [0.5, 0.5, 0.5])
    dev = np.abs(got[:-2] - want).max(1) / hs
    print(f"quadric_core.h vs the oracle: {len(want)} cells, largest deviation {dev.max():.2e} h, {int((dev == 0).sum())} equal bit for bit")
    assert len(want) > 300 and dev.max() < so.POSITION_CAP
