"""csrc/rig_assemble.hip and morig_amd/rigging.py on the device, against the reference's recorded results (tests/golden/rig_assemble_*.npz;
tools/make_rigging_golden.py) and tests/rigging_oracle.py. Everything here is copies and fixed-order float64 sums of identical inputs:
the bar is bit equality, not a tolerance. All fixture cases run as ONE ragged batch, computed once and shared by the tests."""
import numpy as np
import pytest
import torch

import rigging_oracle as ro
from morig_amd import formats, geodesic, rigging, skinning, tracking
from test_rigging_oracle import CASES, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def skeletons():
    return [formats.Rig.from_arrays(c["pos"], c["hier"], c["root_id"], c["names"]) for c in CASES]


def device_weights():
    return cached("w", lambda: [torch.from_numpy(c["weights"]).to(DEV) for c in CASES])


def batch(keep):
    return cached(("batch", keep), lambda: rigging.assemble_rigs(skeletons(), device_weights(), keep_duplicates=keep, entries=True))


@pytest.mark.parametrize("keep,which", [(False, "fin"), (True, "dup")])
def test_dense_skins_equal_the_reference_bit_for_bit(keep, which):
    for rig, c in zip(batch(keep), CASES):
        assert rig.names == c[which + "_names"] and np.array_equal(rig.hierarchy, c[which + "_hier"]) and same_bits(rig.pos, c[which + "_pos"])
        assert same_bits(rig.skins, c[which + "_skins"]), c["name"]
        assert rig.skins_device.is_cuda and same_bits(rig.skins_device.cpu().numpy(), c[which + "_skins"])


def test_rows_past_a_mesh_joint_count_are_zero():
    """the dense block is [N, max J]: a mesh with fewer joints reads zeros there"""
    rigs = batch(False)
    small = rigs[0]                                                                                  # 2 joints, 1 vertex
    block = small.skins_device._base
    assert block.shape == (sum(c["V"] for c in CASES), max(len(r.names) for r in rigs)) and block.shape[1] > len(small.names)
    assert float(block[:small.skins.shape[0], len(small.names):].abs().max()) == 0.0


@pytest.mark.parametrize("keep", [False, True])
def test_device_entries_equal_skin_entries_of_the_dense_result(keep):
    for rig, c in zip(batch(keep), CASES):
        vptr, ev, ej, ew = (t.cpu().numpy() for t in rig.skin_entries_device)
        w_vptr, w_ev, w_ej, w_ew = tracking.skin_entries(rig.skins)
        assert vptr.dtype == np.int32 and np.array_equal(vptr, w_vptr), c["name"]
        assert np.array_equal(ev, w_ev) and np.array_equal(ej, w_ej) and same_bits(ew, w_ew), c["name"]
        o_vptr, o_ev, o_ej, o_ew = ro.entries(rig.skins)
        assert np.array_equal(vptr, o_vptr) and np.array_equal(ev, o_ev) and np.array_equal(ej, o_ej) and same_bits(ew, o_ew)


def test_strided_weights_give_the_bits_of_contiguous_ones():
    """views of a wider block (what skin_weights returns) are read in place; the same numbers in separate tensors are copied"""
    wide = max(c["weights"].shape[1] for c in CASES) + 5
    block = torch.full((sum(c["V"] for c in CASES), wide), 0.5, dtype=torch.float64, device=DEV)
    views, r = [], 0
    for c, w in zip(CASES, device_weights()):
        block[r:r + c["V"], :w.shape[1]] = w
        views.append(block[r:r + c["V"], :w.shape[1]])
        r += c["V"]
    taken = rigging._weight_block(views, torch.device(DEV))
    assert taken.data_ptr() == block.data_ptr() and taken.stride(0) == wide
    strided = rigging.assemble_rigs(skeletons(), views)
    for a, b, c in zip(strided, batch(False), CASES):
        assert same_bits(a.skins, b.skins) and same_bits(a.skins, c["fin_skins"]), c["name"]


def test_two_runs_and_one_mesh_alone_give_the_same_bits():
    again = rigging.assemble_rigs(skeletons(), device_weights(), entries=True)
    for a, b in zip(again, batch(False)):
        assert same_bits(a.skins, b.skins)
        assert all(torch.equal(x, y) for x, y in zip(a.skin_entries_device, b.skin_entries_device))
    i = 7                                                                                            # 48 joints, 257 vertices
    alone, = rigging.assemble_rigs(skeletons()[i:i + 1], device_weights()[i:i + 1])
    assert same_bits(alone.skins, batch(False)[i].skins)


def test_single_mesh_wrappers_on_the_device():
    c = CASES[8]                                                                                     # twins
    skel = skeletons()[8]
    dup = rigging.assemble_skel_skin(skel, c["weights"])
    assert same_bits(dup.skins, c["dup_skins"])
    before = dup.skins.copy()
    fin = rigging.remove_dup_joints(dup)
    assert same_bits(fin.skins, c["fin_skins"]) and same_bits(dup.skins, before) and fin.names == c["fin_names"]


# ---- the stages before it -------------------------------------------------------------------------------------------------------------
def oracle_skins(skel, weights):
    rig = (skel.names, np.asarray(skel.hierarchy), skel.pos, skel.root_id)
    return ro.assemble_rig(rig, weights)


def test_skin_weights_into_assemble_rigs_equals_the_oracle(tmp_path):
    from test_skinning_prep import load_case
    c = load_case("skin_connected", tmp_path)
    _, nn, _, mask, _ = formats.load_skin(c["skin_file"], c["meta"]["k"])
    V, nb = len(c["pos"]), len(c["meta"]["bone_names"])
    up = lambda a: torch.from_numpy(a).to(DEV)
    logits, nn2, mask2 = (np.concatenate([a, a[::-1]], 0) for a in (c["logits"], nn, mask))           # two meshes: views of one block
    tpl = np.concatenate([c["tpl_edge_index"], c["tpl_edge_index"] + V], 1)
    ws = skinning.skin_weights(up(logits), up(nn2), up(mask2), up(tpl), up(np.repeat([0, 1], V)), [nb, nb], mode="joint2rig")
    assert rigging._weight_block(ws, torch.device(DEV)).data_ptr() == ws[0].data_ptr()               # consumed without a copy
    rigs = rigging.assemble_rigs([c["rig"], c["rig"]], ws)
    assert len(rigs[0].names) == len(c["rig"].names) and any("_dup" in n for n in rigging.assembly_plan(c["rig"]).dup.names)
    for rig, w in zip(rigs, ws):
        want = oracle_skins(c["rig"], w.cpu().numpy())
        assert rig.names == want["final"][0] and same_bits(rig.pos, want["final"][2]) and same_bits(rig.skins, want["skins"])
        # nothing is lost here: after the 0.35 x row-max threshold of skin_weights no weight is as small as 1e-5
        assert np.abs(rig.skins.sum(1) - w.cpu().numpy().sum(1)).max() <= 1e-12


def test_predict_rigs_equals_the_stages_called_by_hand(tmp_path):
    from morig_amd import models, synth
    from test_geodesic import load_case as load_geo
    from test_skinning_prep import load_case
    g = load_geo("bone_geo_torus")
    skels = [load_case("skin_connected", tmp_path)["rig"], load_case("skin_fewbones", tmp_path)["rig"]]
    k = geodesic.NUM_NEAREST_BONE
    mesh = synth.make_mesh(g["meta"]["seed"], n_side=g["meta"]["n_side"], with_skin=False)
    assert np.array_equal(mesh.pos.numpy().astype(np.float64), g["pos"])
    kw = dict(nearest_bone=k, use_Dg=True, use_Lf=True, num_keyframes=5, use_motion=True, motion_dim=32, aggr_method="attn")
    net = synth.load_recipe(models.skinnet_motion(**kw).eval(), 204).to(DEV)
    sg = geodesic.surface_geodesic(g["pos"], g["pts"], g["normals"])
    tri = (g["tri_pos"], g["tri_faces"])

    def by_hand(sub):
        inputs, bones = [], []
        for skel in skels:
            bn, _, leaf = skinning.get_bones(skel)
            pos = torch.from_numpy(g["pos"])
            vis = geodesic.bone_visibility(pos if sub is None else pos[torch.from_numpy(sub).long()], bn, *tri)
            geo = geodesic.bone_geodesic_matrix(pos, bn, sg, vis, subsample_ids=sub)
            inputs.append(geodesic.skin_inputs_joint2rig(geo, bn, leaf, k))
            bones.append(bn)
        data = synth.collate([mesh, mesh]).to(DEV)
        data.skin_input = torch.cat([i[0] for i in inputs])
        logits = net(data, data.pred_flow)[2]
        ws = skinning.skin_weights(logits, torch.cat([i[1] for i in inputs]), torch.cat([i[2] for i in inputs]), data.tpl_edge_index,
                                   data.batch, [len(b) for b in bones], mode="joint2rig")
        return [oracle_skins(s, w.cpu().numpy()) for s, w in zip(skels, ws)]

    for sub in (None, g["sub_ids"]):
        data = synth.collate([mesh, mesh]).to(DEV)
        rigs = rigging.predict_rigs(data, skels, net, [sg, sg], [tri, tri], None if sub is None else [sub, sub])
        for rig, want in zip(rigs, by_hand(sub)):
            assert rig.names == want["final"][0] and np.array_equal(rig.hierarchy, want["final"][1])
            assert same_bits(rig.pos, want["final"][2]) and same_bits(rig.skins, want["skins"])
            assert rig.skins.shape == (len(g["pos"]), len(rig.names)) and rig.skins_device.is_cuda
