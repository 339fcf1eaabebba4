"""CPU: tests/transfer_oracle.py against the outputs the reference's transfer_rig_to_remesh recorded (tests/golden/transfer_remesh.npz,
tools/make_transfer_golden.py), its parallel form against its loop, and the closest-point rule against hand-stated answers on a binary
grid."""
import json
import os

import numpy as np
import pytest

import transfer_oracle as to

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transfer_remesh.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    names = json.loads(bytes(z["meta"]).decode())["cases"]
    return {n: {k: z[f"{n}_{k}"] for k in ("vo", "vr", "faces", "skins_ori", "skins", "source")} for n in names}


def case_args(c):
    return c["vo"], c["vr"], c["faces"], c["skins_ori"]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------------- part A
def test_oracle_equals_the_recorded_reference(golden):
    """source_vertex exactly; skins within (2 J 2^-53 + 2^-52) relative: numpy's pairwise row sum and the ascending sum of non-negative
    addends each carry at most (J - 1) 2^-53 relative error, and the division adds half an ulp on each side"""
    assert set(golden) == {"grid_0", "grid_1", "grid_2", "quirk", "chain_down", "chain_up", "root_tie", "underflow"}
    for name, c in golden.items():
        got = to.remesh_loop(*case_args(c))
        assert got["n_unreachable"] == 0 and np.array_equal(got["source"], c["source"]), name
        J = c["skins"].shape[1]
        bound = (2 * J * 2.0 ** -53 + 2.0 ** -52) * np.abs(c["skins"])
        assert got["skins"].shape == c["skins"].shape and np.all(np.abs(got["skins"] - c["skins"]) <= bound), name


def test_golden_cases_are_what_they_are_named_for(golden):
    c = golden["quirk"]
    ref, own = to.remesh_loop(*case_args(c)), to.remesh_loop(*case_args(c), neighbours="faces")
    assert own["n_unreachable"] == 0 and not np.array_equal(ref["source"], own["source"]) and np.array_equal(ref["source"], c["source"])
    down, up = golden["chain_down"], golden["chain_up"]
    V = len(down["vr"])
    assert to.remesh_loop(*case_args(down), neighbours="faces")["n_sweeps"] == V - 1 == 23
    assert to.remesh_loop(*case_args(up), neighbours="faces")["n_sweeps"] == 1
    assert to.remesh_loop(*case_args(down))["n_sweeps"] < V - 1                          # faces 0, 1 and 2 connect everything
    t = golden["root_tie"]
    d0, d1 = to.dist2(t["vr"][2], t["vr"][0]), to.dist2(t["vr"][2], t["vr"][1])
    assert d0 > d1 and np.sqrt(d0) == np.sqrt(d1) and t["source"][2] == 0               # by the squares vertex 1 would have won
    u = golden["underflow"]
    assert u["vr"][0, 0] != u["vo"][1, 0] and np.signbit(u["vo"][1, 2]) and to.dist2(u["vr"][0], u["vo"][1]) == 0.0
    assert to.dist2(u["vr"][0], u["vo"][2]) == 0.0 and u["source"][0] == 1              # the lowest of two coincident originals


def test_neighbour_sets_equal_the_reference_expression():
    _, vr, faces, _ = to.remesh_case(5, 5, 4, seed=3)
    ref, own = to.neighbour_sets(faces, len(vr), "reference"), to.neighbour_sets(faces, len(vr), "faces")
    differ = 0
    for v in range(len(vr)):
        assert np.array_equal(ref[v], to.neighbours_by_argwhere(faces, v))
        assert np.array_equal(own[v], np.setdiff1d(np.unique(faces[np.any(faces == v, 1)]), [v]))
        differ += len(ref[v]) != len(own[v])
    assert differ > 0


@pytest.mark.parametrize("neighbours", ["reference", "faces"])
def test_parallel_form_equals_the_loop(neighbours):
    cases = [to.remesh_case(nx, ny, every, seed) for seed, (nx, ny, every) in enumerate([(4, 4, 3), (6, 5, 7), (8, 3, 24), (5, 9, 45), (7, 7, 10)] * 3)]
    cases += [to.chain_case(17, True), to.chain_case(17, False), to.root_tie_case(), to.underflow_case()]
    vr, faces = to.grid_mesh(4, 4, seed=9)
    lone = np.concatenate([vr, [[5.0, 5.0, 5.0]]])                                      # a vertex in no face: never filled
    cases.append((vr[:2].copy(), lone, faces, to.random_skins(2, 3, 0)))
    deep = 0
    for c in cases:
        loop = to.remesh_loop(*c, neighbours=neighbours)
        source, sweep = to.remesh_parallel(c[0], c[1], c[2], neighbours=neighbours)
        assert np.array_equal(source, loop["source"]) and np.array_equal(sweep, loop["sweep"])
        deep += loop["n_sweeps"] > 2
    assert loop["n_unreachable"] == 1 and loop["sweep"][-1] == -1
    assert deep > 0 or neighbours == "reference"
    near = to.remesh_loop(*cases[-1], neighbours=neighbours, unreachable="nearest")
    assert near["n_unreachable"] == 0 and near["source"][-1] == near["nearest"][-1] >= 0


# ------------------------------------------------------------------------------------------------------------------------- part B
def test_the_seven_regions_on_a_binary_grid():
    for tri, table in ((to.REGION_TRIANGLE, to.REGION_POINTS), (to.DEGENERATE_TRIANGLE, to.DEGENERATE_POINTS)):
        pts = np.array([t[0] for t in table])
        region, bary, d2 = to.closest(pts, tri[None])
        for i, (_, name, want_bary, want_d2) in enumerate(table):
            assert to.REGIONS[region[i, 0]] == name, (i, name)
            assert same(bary[i, 0], np.array(want_bary)) and d2[i, 0] == want_d2, (i, name)
        assert not np.isnan(bary).any() and not np.isnan(d2).any()
    assert {t[1] for t in to.REGION_POINTS} == set(to.REGIONS)
    face, bary, dist, region = to.closest_face([to.COLLAPSED_POINT], to.COLLAPSED_VERTS, to.COLLAPSED_FACES)
    assert face.tolist() == [1] and bary.tolist() == [[0.75, 0.25, 0.0]] and dist.tolist() == [0.5] and to.REGIONS[region[0]] == "edge_ab"


def test_winner_tie_blend_and_a_mesh_without_faces():
    face, bary, dist, region = to.closest_face([to.TIE_POINT], to.TIE_VERTS, to.TIE_FACES)
    assert face.tolist() == [0] and bary.tolist() == [[0.5, 0.0, 0.5]] and dist.tolist() == [0.25] and to.REGIONS[region[0]] == "edge_ac"
    face, *_ = to.closest_face([to.TIE_POINT], to.TIE_VERTS, to.TIE_FACES[::-1])
    assert face.tolist() == [0]                                                        # the lowest face, whichever it is
    S = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.5, 0.5, 0.0]])
    out = to.transfer_skins(to.TIE_VERTS, to.TIE_FACES, S, [to.TIE_POINT, [0.0, 0.0, 0.0]])
    assert same(out["skins"], np.array([[0.5, 0.5, 0.0], [1.0, 0.0, 0.0]]) / (1.0 + 1e-8))
    none = to.transfer_skins(to.TIE_VERTS, np.zeros((0, 3), dtype=np.int64), S, [to.TIE_POINT])
    assert none["face"].tolist() == [-1] and np.isnan(none["bary"]).all() and np.isnan(none["distance"]).all() and not none["skins"].any()


def test_transferred_rows_sum_to_one():
    sv, sf = to.torus(12, 8)
    dv, _ = to.torus(20, 14)
    out = to.transfer_skins(sv, sf, to.random_skins(len(sv), 7, 1), dv)
    assert (out["face"] >= 0).all() and (out["skins"] >= 0).all() and np.abs(out["skins"].sum(1) - 1.0).max() < 1e-7
    assert np.abs(out["bary"].sum(1) - 1.0).max() < 1e-12 and (out["distance"] < 0.1).all() and len(set(out["region"])) >= 3
