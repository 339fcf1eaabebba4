"""CPU: tests/rigging_oracle.py against the reference's recorded results (tests/golden/rig_assemble_*.npz; tools/make_rigging_golden.py),
and the conditions the generator enforces, re-checked on the stored arrays. Everything is copies and fixed-order float64 sums of the same
inputs: the bar is bit equality. The fixtures are loaded once here; the host and GPU tests import them."""
import json
import os

import numpy as np
import pytest

import rigging_oracle as ro

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("pos", "skel_pos", "hier", "weights", "new_of_bone", "dup_hier", "dup_pos", "dup_skins", "fin_hier", "fin_pos", "fin_skins", "rig_txt")


def _load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    out = []
    for i, m in enumerate(meta["cases"]):
        c = dict(m)
        c.update({k: z[f"c{i}_{k}"] for k in KEYS})
        out.append(c)
    return out, meta["gap"]


TREES, GAP = _load("rig_assemble_trees")
DEGENERATE, _ = _load("rig_assemble_degenerate")
CASES = TREES + DEGENERATE
IDS = [c["name"] for c in CASES]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def oracle_rig(c):
    """the skeleton as the pipeline holds it: made from arrays, then one forward pass"""
    hier = np.asarray(c["hier"])
    return (c["names"], hier, ro.rebuild(hier, c["pos"], c["root_id"]), c["root_id"])


def test_the_fixture_set_is_the_one_the_issue_lists():
    assert sorted({(len(c["names"]), c["dtype"]) for c in TREES}) == sorted((j, d) for j in (2, 3, 23, 48) for d in ("float32", "float64"))
    assert {c["V"] for c in TREES} == {1, 63, 65, 257} and all(c["root_id"] != 0 for c in TREES)
    assert [c["name"] for c in DEGENERATE] == ["twins", "leaf_on_parent", "coincident", "child_on_parent", "named_dup"]
    assert "x_dup_0" in DEGENERATE[4]["names"] and "x_dup_0" not in DEGENERATE[4]["fin_names"]
    below = float(np.nextafter(1e-5, 0.0))
    above = float(np.nextafter(1e-5, 1.0))
    w = np.concatenate([c["weights"].reshape(-1) for c in CASES])
    for special in (0.0, 1e-5, below, above, 3e-6):
        assert (w == special).any(), special
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("rig_assemble_")) <= 200 * 1024


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_equals_the_reference(c):
    rig = oracle_rig(c)
    assert same_bits(rig[2], c["skel_pos"])
    got = ro.assemble_rig(rig, c["weights"])
    names, hier, pos, root = got["dup"]
    assert names == c["dup_names"] and np.array_equal(hier, c["dup_hier"]) and root == 0 and same_bits(pos, c["dup_pos"])
    assert np.array_equal(got["new_of_bone"], c["new_of_bone"]) and same_bits(got["dup_skins"], c["dup_skins"])
    names, hier, pos, root = got["final"]
    assert names == c["fin_names"] and np.array_equal(hier, c["fin_hier"]) and root == 0 and same_bits(pos, c["fin_pos"])
    assert same_bits(got["skins"], c["fin_skins"])
    assert str(pos.dtype) == c["dtype"]                                                        # float32 joints stay float32


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_nearest_bone_is_decided_by_a_tie_or_a_gap(c):
    rig = oracle_rig(c)
    old, _ = ro.bones(*rig)
    new, _ = ro.bones(*ro.duplicate(*rig))
    d = np.sort(ro.bone_distances(old, new), axis=1)
    if d.shape[1] > 1:
        assert np.all((d[:, 0] == d[:, 1]) | (d[:, 1] - d[:, 0] > GAP))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_where_the_naive_start_joint_sum_holds_and_where_it_fails(c):
    wrong = int(np.any(ro.naive(oracle_rig(c), c["fin_names"], c["weights"]) != c["fin_skins"], axis=1).sum())
    assert wrong == c["naive_rows"]
    if c in TREES or c["name"] == "child_on_parent":
        assert wrong == 0
    else:
        assert wrong >= 1 and c["naive_differs"]


def test_errors_of_the_oracle():
    with pytest.raises(ValueError):
        ro.bones(["a"], np.array([-1]), np.zeros((1, 3)), 0)
    with pytest.raises(ValueError):                                                            # a "_dup" leaf: nothing to promote
        ro.remove(["a", "a_dup_0"], np.array([-1, 0]), np.zeros((2, 3)), 0, np.zeros((1, 2)))


def test_entries_of_a_dense_matrix():
    x = np.array([[0.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.25, 0.0, 0.75]])
    vptr, ev, ej, ew = ro.entries(x)
    assert vptr.tolist() == [0, 1, 1, 3] and ev.tolist() == [0, 2, 2] and ej.tolist() == [1, 0, 2] and ew.tolist() == [0.5, 0.25, 0.75]
