"""GPU: the skeleton stage (morig_amd/skeleton.py, csrc/skeleton.hip, models/rootnet.py, models/bonenet.py) against the fixtures the
reference's own code made (tests/golden/skel_*.npz; tools/make_skeleton_golden.py).

Criteria: pairs, outside counts, root ids, parents and statuses equal; the inside-share column bit-equal, the distance column within
one float32 ulp; count-derived cost entries and the diagonal bit-equal, -log entries and keys within 1e-14 relative; network logits
within the project's bound (tests/helpers.py), 1e-4 of max(1, scale) or the reference's own float32-against-float64 deviation; end to
end, with tau that bound as an absolute logit error: the root within 2 tau of the reference's best root logit, a spanning tree whose cost
on the reference's cost matrix exceeds the reference tree's by at most 2 (J - 1) tau (|d cost / d logit| <= 1, count entries identical),
the one-call result equal to the staged one bit for bit, and the written file parsing back to the same hierarchy."""
import os

import numpy as np
import pytest
import torch

import skeleton_oracle as sk
from helpers import rel_excess
from morig_amd import formats, geodesic, skeleton, skinning
from test_skeleton_host import net_batch, net_models, net_tolerance, run_both
from test_skeleton_oracle import (MST_CASES, NET_CASES, PAIR_CASES, Vox, bits32, case, check_cost, check_pairs, check_tree, count_mask,
                                  load)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def npy(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- (b) pair geometry
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pair_attributes_equal_reference(name):
    meta, arrs = load("skel_pairs")
    c = case(arrs, name)
    pairs, attr, outside = skeleton.pair_attributes(c["joints"], Vox(arrs["vox_bits"], meta))
    assert pairs.dtype == torch.int64 and attr.dtype == torch.float32 and outside.dtype == torch.int32 and attr.is_cuda
    check_pairs(npy(pairs), npy(attr), npy(outside), c)


def test_pair_attributes_batched_equal_the_single_calls():
    meta, arrs = load("skel_pairs")
    vox = Vox(arrs["vox_bits"], meta)
    cs = [case(arrs, n) for n in PAIR_CASES]
    pairs, attr, outside, pptr = skeleton.pair_attributes_batched([c["joints"] for c in cs], [vox] * len(cs))
    joff = 0
    for b, c in enumerate(cs):
        sl = slice(int(pptr[b]), int(pptr[b + 1]))
        check_pairs(npy(pairs[sl]) - joff, npy(attr[sl]), npy(outside[sl]), c)
        joff += len(c["joints"])


# ---------------------------------------------------------------------------------------------------------------- (c) cost and tree
@pytest.mark.parametrize("name", MST_CASES)
def test_cost_matrix_and_tree_equal_reference(name):
    meta, arrs = load("skel_mst")
    c = case(arrs, name)
    vox = Vox(arrs["vox_bits"], meta)
    j32 = torch.from_numpy(c["joints"]).float().to(DEV)
    (cost,), root = skeleton.connectivity_cost(torch.from_numpy(c["pair_logits"]).to(DEV), torch.from_numpy(c["root_logits"]).to(DEV),
                                               j32, [vox])
    assert cost.dtype == torch.float64 and root.dtype == torch.int32
    check_cost(npy(cost), int(root[0]), c, count_mask(c, vox)[0])
    parent, key = skeleton.prim_mst(cost, int(root[0]))
    assert parent.dtype == torch.int32 and key.dtype == torch.float64
    check_tree(npy(parent), npy(key), c)
    # the reference's own matrix through the device's Prim
    parent, key = skeleton.prim_mst(torch.from_numpy(c["cost"]), int(c["root"]))
    check_tree(npy(parent), npy(key), c)


def test_cost_and_tree_batched_equal_the_single_calls():
    meta, arrs = load("skel_mst")
    vox = Vox(arrs["vox_bits"], meta)
    cs = [case(arrs, n) for n in MST_CASES]
    counts = [len(c["joints"]) for c in cs]
    jb = torch.repeat_interleave(torch.arange(len(cs)), torch.tensor(counts)).to(DEV)
    costs, root = skeleton.connectivity_cost(torch.from_numpy(np.concatenate([c["pair_logits"] for c in cs])).to(DEV).unsqueeze(1),
                                             torch.from_numpy(np.concatenate([c["root_logits"] for c in cs])).to(DEV).unsqueeze(1),
                                             torch.from_numpy(np.concatenate([c["joints"] for c in cs])).float().to(DEV), [vox] * len(cs), jb)
    parents, keys = skeleton.prim_mst(costs, root)
    for b, c in enumerate(cs):
        check_cost(npy(costs[b]), int(root[b]), c, count_mask(c, vox)[0])
        check_tree(npy(parents[b]), npy(keys[b]), c)


def test_disconnected_graph_is_reported_not_returned():
    cost = torch.tensor([[23.0, 1.0, 0.0], [1.0, 23.0, -1e-10], [0.0, -1e-10, 23.0]], dtype=torch.float64, device=DEV)
    assert sk.prim(npy(cost), 0)[2] == 1
    with pytest.raises(RuntimeError, match="disconnected"):
        skeleton.prim_mst(cost, 0)
    with pytest.raises(RuntimeError, match="root"):
        skeleton.prim_mst(cost.abs() + 1.0, 3)


# ---------------------------------------------------------------------------------------------------------------- (a) networks
@pytest.mark.parametrize("name", NET_CASES)
def test_network_logits_equal_reference(name):
    meta, arrs = load("skel_nets")
    data, c = net_batch(meta, arrs, name, DEV)
    outs = run_both(net_models(meta, DEV), meta, data)
    for net in ("rootnet", "bonenet"):
        logits, labels = outs[net]
        ref = torch.from_numpy(c[f"{net}_f32"])
        tol = net_tolerance(c, net)
        print(f"{name}/{net}: max |diff| {float((logits.cpu() - ref).abs().max()):.3e}, bound {tol:.3e} of scale {float(ref.abs().max()):.3f}")
        assert logits.is_cuda and logits.shape == ref.shape and rel_excess(logits, ref, tol, strict=False) <= 0, net


def test_network_random_branches_equal_reference():
    meta, arrs = load("skel_nets")
    data, c = net_batch(meta, arrs, "single", DEV)
    outs = run_both(net_models(meta, DEV), meta, data, "random_torch_seed", True)
    for net in ("rootnet", "bonenet"):
        logits, labels = outs[net]
        assert rel_excess(logits, torch.from_numpy(c[f"{net}_random_f32"]), net_tolerance(c, net), strict=False) <= 0, net
        assert torch.equal(labels.cpu(), torch.from_numpy(c[f"{net}_random_labels"])), net


def net_voxes(meta, c):
    return [Vox(c["vox_bits"][b], meta) for b in range(c["vox_bits"].shape[0])]


@pytest.mark.parametrize("name", NET_CASES)
def test_make_data_equals_create_one_data(name):
    meta, arrs = load("skel_nets")
    want, c = net_batch(meta, arrs, name, DEV)
    counts = meta["cases"][name]["n_joints"]
    jp = np.concatenate([[0], np.cumsum(counts)])
    plain = want.to(DEV)
    for k in ("joints", "pairs", "pair_attr", "joints_batch", "pairs_batch"):
        delattr(plain, k)
    got = skeleton.make_data(plain, [c["joints"][jp[b]:jp[b + 1]] for b in range(len(counts))], net_voxes(meta, c))
    assert torch.equal(got.joints, want.joints) and torch.equal(got.pairs, want.pairs) and got.pairs.dtype == torch.float32
    assert torch.equal(got.joints_batch, want.joints_batch) and torch.equal(got.pairs_batch, want.pairs_batch)
    a, w = npy(got.pair_attr), npy(want.pair_attr)
    assert np.array_equal(bits32(a[:, 1:]), bits32(w[:, 1:])) and int(np.abs(bits32(a[:, 0]).astype(np.int64) - bits32(w[:, 0])).max()) <= 1
    assert got.outside_count.dtype == torch.int32 and got.outside_count.numel() == got.pairs.shape[0]


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", NET_CASES)
def test_predict_skeleton_end_to_end(name, tmp_path):
    meta, arrs = load("skel_nets")
    base, c = net_batch(meta, arrs, name, DEV)
    counts = meta["cases"][name]["n_joints"]
    jp = np.concatenate([[0], np.cumsum(counts)])
    cp = np.concatenate([[0], np.cumsum([n * n for n in counts])])
    voxes = net_voxes(meta, c)
    data = skeleton.make_data(base, [c["joints"][jp[b]:jp[b + 1]] for b in range(len(counts))], voxes)
    models = net_models(meta, DEV)
    torch.manual_seed(meta["torch_seed"])
    rigs = skeleton.predict_skeleton(data, voxes, models["rootnet"], models["bonenet"])
    # staged: the same logits (same seed, same draws) through connectivity_cost and prim_mst, from the grids instead of the stored counts
    outs = run_both(models, meta, data)
    costs, root = skeleton.connectivity_cost(outs["bonenet"][0], outs["rootnet"][0], data.joints, voxes, data.joints_batch)
    parents, _ = skeleton.prim_mst(costs, root)
    assert len(rigs) == len(counts)
    for b, rig in enumerate(rigs):
        J = counts[b]
        assert isinstance(rig, formats.Rig) and rig.names == [f"joint_{i}" for i in range(J)] and rig.pos.dtype == np.float32
        assert rig.root_id == int(root[b]) and np.array_equal(rig.hierarchy, npy(parents[b]))          # one call == staged, bit for bit
        ref_root_logits = c["rootnet_f32"][jp[b]:jp[b + 1], 0].astype(np.float64)
        tau_root = net_tolerance(c, "rootnet") * max(1.0, float(np.abs(c["rootnet_f32"]).max()))
        tau_pair = net_tolerance(c, "bonenet") * max(1.0, float(np.abs(c["bonenet_f32"]).max()))
        assert ref_root_logits[rig.root_id] >= ref_root_logits.max() - 2 * tau_root
        ref_cost = c["ref_cost"][cp[b]:cp[b + 1]].reshape(J, J)
        ref_parent = c["ref_parent"][jp[b]:jp[b + 1]]
        got_total = sk.tree_cost(ref_cost, rig.hierarchy, rig.root_id)                                  # asserts a spanning tree rooted there
        ref_total = sk.tree_cost(ref_cost, ref_parent, int(c["ref_root"][b]))
        print(f"{name}/{b}: J={J} root {rig.root_id} (reference {int(c['ref_root'][b])}), tree cost {got_total:.6f} (reference {ref_total:.6f}), "
              f"same tree: {bool(np.array_equal(rig.hierarchy, ref_parent))}")
        assert got_total <= ref_total + 2 * (J - 1) * tau_pair
        f = str(tmp_path / f"{b}_skel.txt")
        rig.save(f)
        back = formats.Rig(f)
        assert np.array_equal(back.hierarchy, rig.hierarchy) and back.root_id == rig.root_id
        # the next stage takes the rig as it is
        bones, names, leaf = skinning.get_bones(rig)
        pos = base.pos[base.batch == b]
        dist = skinning.volumetric_geodesic(pos, voxes[b], bones)
        assert tuple(dist.shape) == (pos.shape[0], len(bones))
        _, d = geodesic.bone_point_distance(pos.double(), bones)
        assert tuple(d.shape) == (pos.shape[0], len(bones)) and bool(torch.isfinite(d).all())
