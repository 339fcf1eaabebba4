"""GPU: the two visibility rules on the mesh BVH (csrc/bvh.hip) against the brute-force KERNELS they must equal
(morig_scan_visibility, morig_bone_visibility: unchanged) on every case of tests/visibility_cases.py, bit for bit and with no query
excused, and against the oracle of tests/visibility_oracle.py: the masks and the count of box and face tests, test for test
(tests/test_visibility_oracle.py shows on the CPU that the oracle's walk equals its brute force on all of them). Then a view alone against
the batch, chunked against unchunked, two runs, a stale order against a fresh one, and the routes through scan_trajectory and
predict_rigs."""
import functools

import numpy as np
import pytest
import torch

import spatial_oracle as so
import visibility_cases as vc
import visibility_oracle as vo
from morig_amd import geodesic, ragged, rigging, scan, spatial
from morig_amd.runtime import get_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SCAN = {c["name"]: c for c in vc.scan_cases()}
BONE = {c["name"]: c for c in vc.bone_cases()}


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------------- scans
def scan_inputs(c, views=None):
    vs = c["views"] if views is None else [c["views"][v] for v in views]
    return [up(v) for v, _, _ in vs], [up(f) for f in c["faces"]], [vc.camera_of(cam) for _, _, cam in vs], [m for _, m, _ in vs]


def scan_tables(c, tree, cams):
    """the tables of morig_scan_visibility for the views of a ViewBVH"""
    views = np.stack([tree.view_mesh_host, [cm.width for cm in cams], [cm.height for cm in cams], [cm.kind for cm in cams]], 1).astype(np.int32)
    return (tree.verts, tree.vptr, tree.faces, tree.fptr, up(np.stack([cm.row() for cm in cams])), up(views))


def both_scans(c, views=None, order=None):
    """-> (brute-force kernel's vis, the tree's vis, status, visits, the ViewBVH)"""
    ops = get_ops()
    verts, faces, cams, view_mesh = scan_inputs(c, views)
    tree = spatial.build_views(verts, faces, view_mesh)
    if order is not None:
        tree = spatial.ViewBVH(tree.verts, tree.vptr, tree.view_mesh_host, tree.faces, tree.fptr, [len(f) for f in c["faces"]], order)
    tables = scan_tables(c, tree, cams)
    blk, n_blk = ragged.blocks([v.shape[0] for v in verts], ops.SCAN_BLOCK, torch.device(DEV), "test")
    brute = ops.scan_visibility(*tables, blk, n_blk, c["vis_eps"])
    vis, status, visits = ops.bvh_scan_visibility(*tables, c["vis_eps"], tree.order, tree.boxes, tree.node_ptr, tree.flags, True)
    return brute, vis, status, visits, tree


@functools.lru_cache(maxsize=None)
def scan_oracle_walks(name):
    """the oracle's walk of every view of a case, the faces of every mesh ordered on its first view: computed once, never modified"""
    c = SCAN[name] if name in SCAN else vc.scan_bad_face_case()
    orders, out = {}, []
    for v, m, cam in c["views"]:
        if m not in orders:
            orders[m] = vo.mesh_order(v, so.clamped(v, c["faces"][m])[0])
        cm = vc.camera_of(cam)
        out.append(vo.walk_scan(vo.view_tree(v, c["faces"][m], orders[m]), cm.row(), cm.kind, cm.width, cm.height, c["vis_eps"]))
    return out


@pytest.mark.parametrize("name", list(SCAN))
def test_scan_visibility_on_the_tree_equals_the_brute_force_kernel_and_the_oracle(name):
    c = SCAN[name]
    brute, vis, status, visits, _ = both_scans(c)
    assert vis.dtype == torch.uint8 and torch.equal(vis, brute) and int(status) == 0, name
    want = scan_oracle_walks(name)
    assert np.array_equal(vis.cpu().numpy(), np.concatenate([w["vis"] for w in want]))
    assert np.array_equal(visits.cpu().numpy(), np.concatenate([w["visits"] for w in want])), name      # the same traversal, test for test


def test_scan_vertices_outside_the_frustum_walk_nothing():
    c = SCAN["outside_the_frustum"]
    brute, vis, _, visits, _ = both_scans(c)
    seen = np.concatenate([vo.scan_rays(v, vc.camera_of(cam).row(), vc.camera_of(cam).kind, vc.W, vc.H)[3] for v, _, cam in c["views"]])
    assert 0 < seen.sum() < len(seen) and not visits.cpu().numpy()[~seen].any() and visits.cpu().numpy()[seen].all()
    assert not vis.cpu().numpy()[~seen].any()


def test_scan_pruning_stays_under_the_oracles_caps():
    for kind in ("orthographic", "pinhole"):
        _, _, _, visits, _ = both_scans(SCAN[f"torus_4096_{kind}"])
        share = float(visits.sum()) / (visits.numel() * 4096)
        print(f"scan {kind}: {share:.4f} of Q x F (cap {vc.SCAN_CAP[kind]})")
        assert 0 < share < vc.SCAN_CAP[kind]


def test_a_stale_order_gives_the_mask_of_a_fresh_one():
    c = SCAN["torus_4096_stale"]
    brute, stale, _, stale_visits, tree = both_scans(c)                                 # both views in the order of the rest pose
    _, fresh, _, fresh_visits, own = both_scans(c, views=[1])                           # the bent pose ordered on itself
    n = c["views"][0][0].shape[0]
    assert not torch.equal(own.order, tree.order)
    assert torch.equal(stale, brute) and torch.equal(fresh, stale[n:])
    share = float(stale_visits[n:].sum()) / (n * 4096)
    print(f"rest order on the bent pose: {share:.4f} of Q x F (cap {vc.STALE_CAP}); its own order: {float(fresh_visits.sum()) / (n * 4096):.4f}")
    assert 0 < share < vc.STALE_CAP


def test_a_view_alone_gives_the_bits_of_the_batch_and_two_runs_the_same_bits():
    c = vc.scan_batch_case()
    brute, vis, _, visits, tree = both_scans(c)
    again = both_scans(c)
    assert torch.equal(again[1], vis) and torch.equal(again[3], visits) and torch.equal(again[4].boxes.view(torch.int64), tree.boxes.view(torch.int64))
    at = np.concatenate([[0], np.cumsum([len(v) for v, _, _ in c["views"]])])
    for v in range(3):
        _, alone, _, alone_visits, one = both_scans(c, views=[v], order=tree.order)      # the job's order, one view's boxes: a chunk of one view
        assert torch.equal(alone, vis[at[v]:at[v + 1]]) and torch.equal(alone_visits, visits[at[v]:at[v + 1]])
        for k in range(4):
            rows = slice(*tree.node_ptr_host[k, v:v + 2])
            assert torch.equal(one.boxes[one.node_ptr_host[k, 0]:one.node_ptr_host[k, 1]].view(torch.int64), tree.boxes[rows].view(torch.int64))


def test_scan_meshes_with_the_tree_chunked_and_unchunked():
    c = vc.scan_batch_case()
    verts, faces, cams, view_mesh = scan_inputs(c)
    plain = scan.scan_meshes(verts, faces, cams, corr_radius=0.05, view_mesh=view_mesh)
    tree = scan.scan_meshes(verts, faces, cams, corr_radius=0.05, view_mesh=view_mesh, accel="bvh")
    chunked = scan.scan_meshes(verts, faces, cams, corr_radius=0.05, view_mesh=view_mesh, accel="bvh", key_budget=1)
    for a, b, d in zip(plain, tree, chunked):
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, d))
    assert sum(int(s.vismask.sum()) for s in plain) > 0


def test_scan_trajectory_with_the_tree_and_the_bad_face_error():
    v, f = vc.to.torus(32, 16)
    v = v @ vc.sco.rotation(5).T
    traj = up(np.stack([v, vc.bent(v, 30.0), vc.bent(v, 70.0)], 1))
    cams = [vc.camera_of(cam) for cam in vc.cameras(64, 48)]
    plain = scan.scan_trajectory([traj, traj], [up(f), up(f)], cams, n_pts=64)
    tree = scan.scan_trajectory([traj, traj], [up(f), up(f)], cams, n_pts=64, accel="bvh")
    for a, b in zip(plain, tree):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert 0 < int(plain[0][1].sum()) < plain[0][1].numel()
    bad = vc.scan_bad_face_case()
    verts, faces, cm, view_mesh = scan_inputs(bad)
    errors = []
    for accel in (None, "bvh"):
        with pytest.raises(ValueError, match="outside its mesh") as e:
            scan.scan_meshes(verts, faces, cm, view_mesh=view_mesh, accel=accel)
        errors.append(str(e.value))
    assert errors[0] == errors[1]
    brute, vis, status, visits, tree = both_scans(bad)                                  # the clamped faces take part, the status says so
    assert torch.equal(vis, brute) and int(status) == get_ops().SCAN_BAD_FACE and tree.flags.tolist() == [get_ops().BVH_BAD_FACE]
    want, = scan_oracle_walks("bad_face")
    assert want["bad"] and np.array_equal(vis.cpu().numpy(), want["vis"]) and np.array_equal(visits.cpu().numpy(), want["visits"])


# ------------------------------------------------------------------------------------------------------------------------- bones
def bone_columns(c):
    return [[up(m[k]) for m in c["meshes"]] for k in range(4)]


def bone_on_the_tree(c):
    """-> (vis, status, visits) of morig_bvh_bone_visibility on the batch of a case"""
    pos, bones, tri_pos, tri_faces = bone_columns(c)
    pr = geodesic._Pairs(pos, bones, "test").to(torch.device(DEV))
    tree = spatial.build(tri_pos, tri_faces)
    m = tree.mesh
    return get_ops().bvh_bone_visibility(pr.d_pos, pr.vtx_ptr, pr.d_bones, pr.bone_ptr, m.verts, m.vptr, m.faces, m.fptr, pr.d_off, pr.n, tree.order,
                                         tree.boxes, tree.node_ptr, tree.flags, True)


@functools.lru_cache(maxsize=None)
def bone_oracle_walks(name):
    return [vo.walk_bone(so.build(t, f), p, b) for p, b, t, f in BONE[name]["meshes"]]


@pytest.mark.parametrize("name", list(BONE))
def test_bone_visibility_on_the_tree_equals_the_brute_force_kernel_and_the_oracle(name):
    c = BONE[name]
    cols = bone_columns(c)
    plain = geodesic.bone_visibility_batched(*cols)
    tree = geodesic.bone_visibility_batched(*cols, accel="bvh")
    assert all(a.dtype == torch.bool and torch.equal(a, b) for a, b in zip(plain, tree)), name
    vis, status, visits = bone_on_the_tree(c)
    assert int(status) == 0 and torch.equal(vis.bool(), torch.cat([t.reshape(-1) for t in tree]))
    want = bone_oracle_walks(name)
    assert np.array_equal(vis.cpu().numpy(), np.concatenate([w["vis"] for w in want]))
    assert np.array_equal(visits.cpu().numpy(), np.concatenate([w["visits"] for w in want])), name      # the same traversal, test for test


def test_bone_pruning_a_mesh_alone_the_two_orders_and_two_runs():
    c = BONE["torus_own_occluder"]
    vis, _, visits = bone_on_the_tree(c)
    share = float(visits.sum()) / (visits.numel() * len(c["meshes"][0][3]))
    print(f"bone: {share:.4f} of Q x F (cap {vc.BONE_CAP})")
    assert 0 < share < vc.BONE_CAP and 0 < int(vis.sum()) < vis.numel()
    forward, backward = (bone_on_the_tree(BONE[n]) for n in ("ragged", "ragged_reversed"))
    again = bone_on_the_tree(BONE["ragged"])
    assert torch.equal(again[0], forward[0]) and torch.equal(again[2], forward[2])
    sizes = [len(m[0]) * len(m[1]) for m in BONE["ragged"]["meshes"]]
    at = np.concatenate([[0], np.cumsum(sizes)])
    back = np.concatenate([[0], np.cumsum(sizes[::-1])])
    for b in range(len(sizes)):
        r = len(sizes) - 1 - b
        assert torch.equal(forward[0][at[b]:at[b + 1]], backward[0][back[r]:back[r + 1]])
        assert torch.equal(forward[2][at[b]:at[b + 1]], backward[2][back[r]:back[r + 1]])
        alone = geodesic.bone_visibility(*(up(x) for x in BONE["ragged"]["meshes"][b]), accel="bvh")
        assert torch.equal(alone.reshape(-1), forward[0][at[b]:at[b + 1]].bool())


def test_predict_rigs_with_the_tree_equals_predict_rigs_without(tmp_path):
    from morig_amd import models, synth
    from test_geodesic import load_case as load_geo
    from test_skinning_prep import load_case
    g = load_geo("bone_geo_torus")
    skels = [load_case("skin_connected", tmp_path)["rig"], load_case("skin_fewbones", tmp_path)["rig"]]
    mesh = synth.make_mesh(g["meta"]["seed"], n_side=g["meta"]["n_side"], with_skin=False)
    kw = dict(nearest_bone=geodesic.NUM_NEAREST_BONE, use_Dg=True, use_Lf=True, num_keyframes=5, use_motion=True, motion_dim=32, aggr_method="attn")
    net = synth.load_recipe(models.skinnet_motion(**kw).eval(), 204).to(DEV)
    sg = geodesic.surface_geodesic(g["pos"], g["pts"], g["normals"])
    tri = (g["tri_pos"], g["tri_faces"])
    for sub in (None, g["sub_ids"]):
        rigs = [rigging.predict_rigs(synth.collate([mesh, mesh]).to(DEV), skels, net, [sg, sg], [tri, tri], None if sub is None else [sub, sub],
                                     accel=accel) for accel in (None, "bvh")]
        for a, b in zip(*rigs):
            assert a.names == b.names and torch.equal(a.skins_device, b.skins_device)
    with pytest.raises(ValueError, match='accel is None or "bvh"'):
        rigging.predict_rigs(synth.collate([mesh, mesh]).to(DEV), skels, net, [sg, sg], [tri, tri], accel="grid")
