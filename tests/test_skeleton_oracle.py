"""tests/skeleton_oracle.py against the fixtures the reference's own code made (tools/make_skeleton_golden.py), the conditions those
fixtures were made under, the rig writer, the library's exports and the two networks' state-dict layout. No GPU.

Criteria (the device tests are held to the same): pairs, outside counts, root id, parents equal; the inside-share column bit-equal as
float32, the distance column within one float32 ulp; cost entries that come from counts (halved ones included) and the diagonal
bit-equal, -log entries and keys within 1e-14 relative."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import skeleton_oracle as sk  # noqa: E402
from morig_amd import formats  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PAIR_CASES = ("inside", "hole", "outside_grid", "zero_length", "plane")
MST_CASES = ("ties", "saturated", "plane", "two", "fortyeight")
NET_CASES = ("single", "ragged")


class Vox:
    """binvox-like grid as the reference reads it (data, translate, scale, dims)"""

    def __init__(self, bits, meta):
        self.data = np.unpackbits(np.asarray(bits))[:88 ** 3].reshape(88, 88, 88).astype(bool)
        self.translate, self.scale, self.dims = list(meta["translate"]), float(meta["scale"]), list(meta["dims"])


def load(name):
    """-> (meta, {key: numpy array})"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode()), {k: z[k] for k in z.files if k != "meta"}


def case(arrs, name):
    return {k[len(name) + 1:]: v for k, v in arrs.items() if k.startswith(name + "_")}


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def ulp_distance_f32(a, b):
    """distance in float32 units in the last place between same-sign finite values"""
    ia, ib = bits32(a).astype(np.int64), bits32(b).astype(np.int64)
    return np.abs(ia - ib)


def check_pairs(got_pairs, got_attr, got_outside, c):
    """criteria 1 and 2 against one case of skel_pairs"""
    assert np.array_equal(np.asarray(got_pairs), c["pairs"])
    assert np.array_equal(np.asarray(got_outside), c["outside"])
    got_attr = np.asarray(got_attr, dtype=np.float32)
    assert np.array_equal(bits32(got_attr[:, 1]), bits32(c["pair_attr"][:, 1]))
    assert np.array_equal(got_attr[:, 2], c["pair_attr"][:, 2])
    assert int(ulp_distance_f32(got_attr[:, 0], c["pair_attr"][:, 0]).max(initial=0)) <= 1


def count_mask(c, vox):
    """which entries of a skel_mst case's cost matrix come from outside-sample counts (and the diagonal): by the oracle's counts, which
    test_oracle_pair_attributes_equal_reference holds to the reference's"""
    o = sk.pair_attributes(c["joints"], vox.data, vox.translate, vox.scale, vox.dims[0])
    mask = np.eye(len(c["joints"]), dtype=bool)
    for (i, j), n_out in zip(o["pairs"], o["outside_count"]):
        mask[i, j] = mask[j, i] = n_out > 1
    return mask, o["outside_count"]


def check_cost(got_cost, got_root, c, from_count):
    """criteria 1 and 3 against one case of skel_mst"""
    ref = c["cost"]
    got = np.asarray(got_cost, dtype=np.float64).reshape(ref.shape)
    assert int(got_root) == int(c["root"])
    assert np.array_equal(bits64(got[from_count]), bits64(ref[from_count]))
    rest = ~from_count
    assert np.all(np.abs(got[rest] - ref[rest]) <= 1e-14 * np.abs(ref[rest]))


def check_tree(got_parent, got_key, c):
    assert np.array_equal(np.asarray(got_parent).astype(np.int64), c["parent"].astype(np.int64))
    k, r = np.asarray(got_key, dtype=np.float64), c["key"]
    assert np.all(np.abs(k - r) <= 1e-14 * np.abs(r))


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", PAIR_CASES)
def test_oracle_pair_attributes_equal_reference(name):
    meta, arrs = load("skel_pairs")
    c = case(arrs, name)
    vox = Vox(arrs["vox_bits"], meta)
    o = sk.pair_attributes(c["joints"], vox.data, vox.translate, vox.scale, vox.dims[0])
    check_pairs(o["pairs"], o["pair_attr"], o["outside_count"], c)


@pytest.mark.parametrize("name", MST_CASES)
def test_oracle_cost_and_tree_equal_reference(name):
    meta, arrs = load("skel_mst")
    c = case(arrs, name)
    vox = Vox(arrs["vox_bits"], meta)
    mask, outside = count_mask(c, vox)
    cost, root, from_count = sk.connectivity_cost(c["pair_logits"], c["root_logits"], c["joints"].astype(np.float32), outside)
    assert np.array_equal(mask, from_count)
    check_cost(cost, root, c, mask)
    parent, key, status, _ = sk.prim(cost, root)
    assert status == 0
    check_tree(parent, key, c)
    assert sk.tree_cost(c["cost"], parent, root) == pytest.approx(float(c["key"].sum()), rel=1e-12)


def test_oracle_reports_a_disconnected_graph():
    cost = np.array([[23.0, 1.0, 0.0], [1.0, 23.0, -1e-10], [0.0, -1e-10, 23.0]])
    parent, _, status, _ = sk.prim(cost, 0)
    assert parent is None and status == 1


# ---------------------------------------------------------------------------------------------------------------- fixture conditions
def test_fixture_conditions_hold():
    meta, arrs = load("skel_pairs")
    m = meta["margins"]
    assert meta["numpy"].split(".")[0] == "2"                  # the float32 chain of the cost loop is NumPy 2's (NEP 50)
    vox = Vox(arrs["vox_bits"], meta)
    for name in PAIR_CASES:
        o = sk.pair_attributes(case(arrs, name)["joints"], vox.data, vox.translate, vox.scale, vox.dims[0])
        assert o["length_margin"] >= m["length"] and o["voxel_margin"] >= m["voxel"], name
    meta, arrs = load("skel_mst")
    vox = Vox(arrs["vox_bits"], meta)
    for name in MST_CASES:
        c = case(arrs, name)
        o = sk.pair_attributes(c["joints"], vox.data, vox.translate, vox.scale, vox.dims[0])
        assert o["length_margin"] >= m["length"] and o["voxel_margin"] >= m["voxel"], name
        _, _, status, info = sk.prim(c["cost"], int(c["root"]))
        assert status == 0 and info["margin"] >= m["key"] and info["ties_integer"], name
        assert sk.root_margin(c["root_logits"]) >= m["key"], name
        # the probabilities torch computed for the reference are the correctly rounded ones
        assert np.array_equal(bits32(c["prob"]), bits32(sk.sigmoid_f32(c["pair_logits"]))), name
    ties = case(arrs, "ties")
    k = np.delete(ties["key"], int(ties["root"]))
    assert len(np.unique(k)) < len(k) and meta["notes"]["saturated"]["no_edge"] >= 2 and meta["notes"]["plane"]["halved"] >= 3
    assert (case(arrs, "saturated")["cost"] <= 0).sum() >= 4
    assert case(arrs, "two")["cost"].shape == (2, 2) and case(arrs, "fortyeight")["cost"].shape == (48, 48)
    meta, arrs = load("skel_nets")
    assert sorted(meta["cases"]["ragged"]["n_joints"]) == [2, 17, 48]
    for name in NET_CASES:
        c = case(arrs, name)
        jp = np.concatenate([[0], np.cumsum(meta["cases"][name]["n_joints"])])
        for b in range(len(jp) - 1):
            vox = Vox(c["vox_bits"][b], meta)
            o = sk.pair_attributes(c["joints"][jp[b]:jp[b + 1]], vox.data, vox.translate, vox.scale, vox.dims[0])
            assert o["length_margin"] >= m["length"] and o["voxel_margin"] >= m["voxel"], (name, b)


# ---------------------------------------------------------------------------------------------------------------- the rig writer
@pytest.mark.parametrize("name", MST_CASES)
def test_rig_from_arrays_writes_the_reference_file(name, tmp_path):
    _, arrs = load("skel_mst")
    c = case(arrs, name)
    rig = formats.Rig.from_arrays(c["joints"].astype(np.float32), c["parent"], int(c["root"]))
    assert rig.pos.dtype == np.float32 and np.array_equal(bits32(rig.pos), bits32(c["rig_pos"]))
    assert np.array_equal(bits64(rig.offset), bits64(c["rig_offset"]))
    assert rig.names == [f"joint_{i}" for i in range(len(c["parent"]))] and rig.root_name == f"joint_{int(c['root'])}"
    f = str(tmp_path / "skel.txt")
    rig.save(f)
    assert open(f, "rb").read() == bytes(c["skel_txt"])
    back = formats.Rig(f)
    assert np.array_equal(back.hierarchy, c["parent"]) and back.root_id == int(c["root"]) and back.names == rig.names
    assert np.abs(back.pos - c["rig_pos"]).max() <= 1e-7
    if "skins" in c:
        rig = formats.Rig.from_arrays(c["joints"].astype(np.float32), c["parent"], int(c["root"]), skins=c["skins"])
        rig.save(f)
        assert open(f, "rb").read() == bytes(c["rig_txt"])
        assert np.array_equal(formats.Rig(f).skins, c["skins"])


def test_rig_from_arrays_refuses_what_is_not_a_rooted_tree():
    pos = np.zeros((3, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        formats.Rig.from_arrays(pos, [-1, 2, 1], 0)                # a cycle the root does not reach
    with pytest.raises(ValueError):
        formats.Rig.from_arrays(pos, [-1, -1, 0], 0)               # two roots
    with pytest.raises(ValueError):
        formats.Rig.from_arrays(pos, [-1, 0, 5], 0)


def test_predicted_rig_feeds_the_skinning_stage():
    from morig_amd import skinning
    _, arrs = load("skel_mst")
    c = case(arrs, "plane")
    rig = formats.Rig.from_arrays(c["joints"].astype(np.float32), c["parent"], int(c["root"]))
    bones, names, leaf = skinning.get_bones(rig)
    n_leaf = sum(1 for v in range(len(c["parent"])) if v not in set(c["parent"].tolist()))
    assert bones.shape == (len(c["parent"]) - 1 + n_leaf, 6) and bones.dtype == np.float64 and sum(leaf) == n_leaf
    assert np.array_equal(skinning.start_joints(rig, names), [rig.names.index(n[0]) for n in names])


# ---------------------------------------------------------------------------------------------------------------- library and modules
def test_library_exports_the_skeleton_entry_points():
    from morig_amd import native
    lib = native.load_library()
    for name in ("morig_pair_attr", "morig_skeleton_cost", "morig_prim_mst"):
        assert name in native.EXPORTS and hasattr(lib, name)
    assert lib.morig_abi_version() == 3
    header = open(os.path.join(ROOT, "include", "morig_hip.h")).read()
    assert "#define MORIG_ABI_VERSION 3" in header and "int morig_prim_mst(" in header


@pytest.mark.parametrize("net", ("rootnet", "bonenet"))
def test_state_dict_layout_equals_the_reference(net):
    from morig_amd.models import bonenet, rootnet
    meta, _ = load("skel_nets")
    model = {"rootnet": rootnet.ROOTNET, "bonenet": bonenet.PairCls}[net]()
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert got == meta["nets"][net]["state_dict"]
    sd = {k: torch.zeros(s) if not k.endswith("num_batches_tracked") else torch.zeros(s, dtype=torch.long) for k, s in meta["nets"][net]["state_dict"]}
    model.load_state_dict(sd, strict=True)
