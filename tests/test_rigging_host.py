"""CPU: the host side of morig_amd/rigging.py -- the plan builder, the CSR tables, their concatenation over a ragged batch and the
slicing of the results -- with the two kernels emulated in numpy (tests/rigging_emulate.py through ``runtime._test_ops``), against the
reference's recorded results (tests/golden/rig_assemble_*.npz). Everything is compared bit for bit."""
import numpy as np
import pytest
import torch

import rigging_emulate
import rigging_oracle as ro
from morig_amd import formats, rigging, runtime, tracking
from test_rigging_oracle import CASES, DEGENERATE, IDS, TREES, same_bits


@pytest.fixture()
def ops(monkeypatch):
    o = rigging_emulate.RigOps()
    monkeypatch.setattr(runtime, "_test_ops", o)
    return o


def skeleton(c):
    return formats.Rig.from_arrays(c["pos"], c["hier"], c["root_id"], c["names"])


def check_rig(rig, c, which):
    assert rig.names == c[which + "_names"] and np.array_equal(rig.hierarchy, c[which + "_hier"]) and rig.root_id == 0
    assert rig.root_name == c["names"][c["root_id"]]
    assert same_bits(rig.pos, c[which + "_pos"]) and same_bits(rig.skins, c[which + "_skins"])


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_plan_replays_the_reference_bookkeeping(c):
    skel = skeleton(c)
    assert same_bits(skel.pos, c["skel_pos"])
    plan = rigging.assembly_plan(skel)
    assert plan.dup.names == c["dup_names"] and np.array_equal(plan.dup.hierarchy, c["dup_hier"]) and same_bits(plan.dup.pos, c["dup_pos"])
    assert np.array_equal(plan.new_of_bone, c["new_of_bone"])
    assert plan.final.names == c["fin_names"] and np.array_equal(plan.final.hierarchy, c["fin_hier"]) and same_bits(plan.final.pos, c["fin_pos"])
    want = ro.assemble_rig((c["names"], np.asarray(c["hier"]), c["skel_pos"], c["root_id"]), c["weights"])["segments"]
    assert plan.segments == want and all(seg[0] == plan.dup.names.index(n) for seg, n in zip(plan.segments, plan.final.names))
    seg_ptr, bone_ptr, bones = plan.tables()
    assert seg_ptr[-1] == sum(len(s) for s in want) == len(bone_ptr) - 1 and bone_ptr[-1] == len(bones) <= len(plan.new_of_bone)
    for s in range(len(bone_ptr) - 1):
        assert (np.diff(bones[bone_ptr[s]:bone_ptr[s + 1]]) > 0).all()                             # ascending inside a segment
    assert sorted(bones.tolist()) == sorted(i for i, n in enumerate(plan.new_of_bone) if any(n in seg for seg in want))
    k_ptr, kb_ptr, k_bones = plan.tables(keep_duplicates=True)
    assert np.array_equal(k_ptr, np.arange(len(c["dup_names"]) + 1)) and sorted(k_bones.tolist()) == list(range(len(plan.new_of_bone)))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_one_mesh_equals_the_reference_and_its_rig_file(ops, c, tmp_path):
    skel = skeleton(c)
    rig, = rigging.assemble_rigs([skel], [c["weights"]])
    check_rig(rig, c, "fin")
    assert ops.calls == ["rig_assemble"] and same_bits(rig.skins_device.numpy(), c["fin_skins"])
    path = str(tmp_path / "0_rig.txt")
    rig.save(path)
    assert open(path, "rb").read() == c["rig_txt"].tobytes()
    back = formats.Rig(path)
    assert back.names == rig.names and np.array_equal(back.hierarchy, rig.hierarchy) and back.root_id == 0
    assert np.array_equal(back.skins > 0, np.round(rig.skins, 4) > 0) and np.abs(back.skins - rig.skins).max(initial=0) <= 5.0001e-5
    dup, = rigging.assemble_rigs([skel], [torch.from_numpy(c["weights"])], keep_duplicates=True)
    check_rig(dup, c, "dup")


def test_ragged_batch_with_entries(ops):
    picked = [TREES[0], DEGENERATE[2], TREES[4], TREES[7], DEGENERATE[0], TREES[2], DEGENERATE[4]]
    rigs = rigging.assemble_rigs([skeleton(c) for c in picked], [c["weights"] for c in picked], entries=True)
    assert ops.calls == ["rig_assemble", "rig_skin_counts", "rig_skin_fill"]
    for rig, c in zip(rigs, picked):
        check_rig(rig, c, "fin")
        vptr, ev, ej, ew = (t.numpy() for t in rig.skin_entries_device)
        w_vptr, w_ev, w_ej, w_ew = tracking.skin_entries(c["fin_skins"])
        assert vptr.dtype == np.int32 and np.array_equal(vptr, w_vptr) and np.array_equal(ev, w_ev) and np.array_equal(ej, w_ej)
        assert same_bits(ew, w_ew)
    kept = rigging.assemble_rigs([skeleton(c) for c in picked], [c["weights"] for c in picked], keep_duplicates=True)
    for rig, c in zip(kept, picked):
        check_rig(rig, c, "dup")


def test_views_of_one_block_are_read_in_place(ops):
    """what skin_weights returns: row ranges of one [N, max n_bones] block, the first n_bones columns of each"""
    picked = [TREES[0], TREES[5], TREES[1], DEGENERATE[1]]                                        # the first one a single vertex
    wide = max(c["weights"].shape[1] for c in picked) + 3
    block = torch.full((sum(c["V"] for c in picked), wide), 7.0, dtype=torch.float64)
    views, r = [], 0
    for c in picked:
        block[r:r + c["V"], :c["weights"].shape[1]] = torch.from_numpy(c["weights"])
        views.append(block[r:r + c["V"], :c["weights"].shape[1]])
        r += c["V"]
    rigs = rigging.assemble_rigs([skeleton(c) for c in picked], views)
    assert ops.last_W.data_ptr() == block.data_ptr() and ops.last_W.stride(0) == wide                # no copy
    for rig, c in zip(rigs, picked):
        check_rig(rig, c, "fin")
    rigs = rigging.assemble_rigs([skeleton(c) for c in picked], [v.clone() for v in views])           # separate storages: one new block
    assert ops.last_W.data_ptr() != block.data_ptr()
    for rig, c in zip(rigs, picked):
        check_rig(rig, c, "fin")
    rigs = rigging.assemble_rigs([skeleton(c) for c in picked[::-1]], views[::-1])                    # one storage, another order: copied
    assert ops.last_W.data_ptr() != block.data_ptr()
    for rig, c in zip(rigs, picked[::-1]):
        check_rig(rig, c, "fin")


@pytest.mark.parametrize("c", DEGENERATE + TREES[4:6], ids=IDS[8:] + IDS[4:6])
def test_single_mesh_wrappers_keep_the_reference_signatures(ops, c):
    skel = skeleton(c)
    dup = rigging.add_duplicate_joints(skel)
    assert dup.names == c["dup_names"] and same_bits(dup.pos, c["dup_pos"])
    bones_old, bones_new = rigging._bones(skel)[0], rigging._bones(dup)[0]
    assert str(bones_old.dtype) == c["dtype"] and same_bits(bones_old.astype(np.float64), rigging.skinning.get_bones(skel)[0])
    bone_map = rigging.mapping_bone_index(bones_old, bones_new)
    names_new = rigging._bones(dup)[1]
    assert [dup.names.index(names_new[bone_map[i]][0]) for i in range(len(bones_old))] == c["new_of_bone"].tolist()
    with_skins = rigging.assemble_skel_skin(skel, c["weights"])
    check_rig(with_skins, c, "dup")
    before = with_skins.skins.copy()
    final = rigging.remove_dup_joints(with_skins)
    check_rig(final, c, "fin")
    assert same_bits(with_skins.skins, before)                                                        # the reference adds in place; this does not


def test_remove_dup_joints_adds_raw_columns(ops):
    """on its own the function sums whatever the columns hold: no 1e-5 threshold there"""
    c = DEGENERATE[0]
    rig = rigging.assemble_skel_skin(skeleton(c), c["weights"])
    rig.skins = np.random.default_rng(3).uniform(-1e-5, 1e-5, rig.skins.shape)
    got = rigging.remove_dup_joints(rig)
    want = ro.remove(rig.names, np.asarray(rig.hierarchy), rig.pos, 0, rig.skins)[1]
    assert same_bits(got.skins, want)


def test_value_errors(ops):
    one = formats.Rig.from_arrays(np.zeros((1, 3)), [-1], 0)
    with pytest.raises(ValueError, match="no bones"):
        rigging.assembly_plan(one)
    with pytest.raises(ValueError, match="no bones"):
        rigging.assemble_rigs([one], [np.zeros((4, 0))])
    leaf_dup = formats.Rig.from_arrays(np.arange(9.0).reshape(3, 3), [-1, 0, 1], 0, ["r", "a", "a_dup_0"])
    with pytest.raises(ValueError, match="no child to promote"):
        rigging.assembly_plan(leaf_dup)
    leaf_dup.skins = np.zeros((2, 3))
    with pytest.raises(ValueError, match="no child to promote"):
        rigging.remove_dup_joints(leaf_dup)
    c = TREES[2]
    with pytest.raises(ValueError, match="one column per bone"):
        rigging.assemble_rigs([skeleton(c)], [c["weights"][:, :-1]])
    with pytest.raises(ValueError, match="one weight matrix per skeleton"):
        rigging.assemble_rigs([skeleton(c)], [])
    clash = formats.Rig.from_arrays(np.arange(9.0).reshape(3, 3), [-1, 0, 0], 0, ["r", "r_dup_0", "b"])
    with pytest.raises(ValueError):                                                                   # a child named like the duplicate made for it
        rigging.assembly_plan(clash)
    assert ops.calls == []


def test_new_symbols_declared_and_exported():
    import os
    import re
    from morig_amd import native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "morig_hip.h")).read(), flags=re.S)
    lib = native.load_library()
    for s in ("morig_rig_assemble", "morig_rig_skin_entries"):
        assert re.search(r"\b" + s + r"\s*\(", hdr) and s in native.EXPORTS and hasattr(lib, s)
    assert native.ABI_VERSION == 3 and lib.morig_abi_version() == 3 and native.NativeOps.RIG_RAW == 1
    names = [lib.morig_prof_name(k) for k in range(native._K["MORIG_PROF_KINDS"])]
    assert b"rig_assemble" in names and b"rig_skin_entries" in names
