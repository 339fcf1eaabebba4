"""CPU: the host logic of morig_amd/spatial.py and of the ``accel`` routes of labels.py / transfer.py on an emulated op layer
(tests/spatial_emulate.py through ``runtime._test_ops``): level tables and node ranges, the stable order, the refit, the per-mesh views,
the refusals, the status handling, what is launched with and without ``accel``; and csrc/bvh_core.h with the two rule headers as the
stand-alone program tools/bvh_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import labels_oracle as lo
import spatial_cases as sc
import spatial_emulate as se
import spatial_oracle as so
import transfer_oracle as to
from morig_amd import abi, labels, native, runtime, spatial, transfer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops():
    emu = se.SpatialOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def meshes_of(case):
    return [torch.from_numpy(v) for v, _ in case["meshes"]], [torch.from_numpy(f) for _, f in case["meshes"]]


# ------------------------------------------------------------------------------------------------------------------------- host program
def test_the_entering_rules_and_the_serial_walks_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "bvh_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "bvh_host_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "" and done.stdout.strip().endswith("ok"), (done.returncode, done.stdout[-2000:], done.stderr[-2000:])


def test_the_c_abi_declares_types_and_refuses_without_a_device():
    names = ["morig_bvh_build_keys", "morig_bvh_boxes", "morig_bvh_ray_cast", "morig_bvh_closest", "morig_bvh_blocked"]
    assert set(names) <= set(native.EXPORTS) and len(abi.STRUCTS) == 8                 # plain parameters: no new argument struct
    lib, K = native.load_library(), abi.CONSTANTS
    assert K["MORIG_BVH_MAX_FACES"] == spatial.MAX_FACES == 64 ** 4 and K["MORIG_BVH_BAD_FACE"] == se.SpatialOps.BVH_BAD_FACE
    none = [None] * 4
    assert lib.morig_bvh_boxes(*none, 1, 64 ** 4 + 1, None, None, 1, 0, 0, 0, None, None, None) == K["MORIG_E_UNSUPPORTED"]   # before anything is launched
    assert lib.morig_bvh_boxes(*none, 1, 10, None, None, -1, 0, 0, 0, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_bvh_boxes(*none, 1, 10, None, None, 1, 0, 0, 0, None, None, None) == K["MORIG_E_INVALID"]            # no flag words
    assert lib.morig_bvh_boxes(*none, 0, 0, None, None, 0, 0, 0, 0, None, None, None) == K["MORIG_OK"]                   # no mesh
    assert lib.morig_bvh_build_keys(*none[:3], 0, None, 0, None, None, None) == K["MORIG_OK"]                             # no face
    assert lib.morig_bvh_build_keys(*none[:3], 5, None, 1, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_bvh_build_keys(*none[:3], -1, None, 1, None, None, None) == K["MORIG_E_INVALID"]
    tree = [None] * 4 + [1] + [None] * 4                                                # verts .. fptr, n_meshes, order .. flags
    assert lib.morig_bvh_ray_cast(None, None, None, 4, *tree, 0, None, None, None, None, None, None) == K["MORIG_E_INVALID"]    # no status word
    assert lib.morig_bvh_ray_cast(None, None, None, 4, *tree, 2, None, None, None, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_bvh_closest(None, None, 0, *tree, None, None, None, None, None, None) == K["MORIG_OK"]                # no point
    assert lib.morig_bvh_closest(None, None, 3, *tree, None, None, None, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_bvh_closest(None, None, -1, *tree, None, None, None, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_bvh_blocked(None, None, None, 4, None, None, *tree, None, None, None, None) == K["MORIG_E_INVALID"]   # no status word
    prof = [lib.morig_prof_name(k) for k in range(K["MORIG_PROF_KINDS"])]
    assert b"bvh_build" in prof and b"bvh_query" in prof


# ------------------------------------------------------------------------------------------------------------------------- tables
def test_level_and_node_tables():
    nf = np.array([0, 1, 64, 65, 4096, 4097, 64 ** 3 + 1, 0])
    counts = spatial.level_table(nf)
    for b, n in enumerate(nf):
        want = so.level_counts(n)
        assert list(counts[:len(want), b]) == want and np.all(counts[len(want):, b] == 0)
    ptr, totals = spatial.node_table(nf)
    assert ptr.shape == (4, len(nf) + 1) and list(totals) == list(counts.sum(1))
    assert ptr[0, 0] == 0 and all(ptr[k, -1] == ptr[k + 1, 0] for k in range(3)) and ptr[3, -1] == totals.sum()
    assert np.array_equal(np.diff(ptr, axis=1), counts)


def test_build_launches_keys_one_sort_and_boxes_and_reads_nothing(ops):
    case = sc.ragged_case()
    verts, faces = meshes_of(case)
    bvh = spatial.build(verts, faces)
    assert ops.calls == ["mesh_bbox", "bvh_build_keys", "bvh_boxes"]
    fp = bvh.mesh.fptr_host
    for b, (v, f) in enumerate(case["meshes"]):
        tree = so.build(v, f) if len(v) else dict(order=np.zeros(0, dtype=np.int64), levels=[])
        assert np.array_equal(bvh.order.numpy()[fp[b]:fp[b + 1]] - fp[b], tree["order"])            # the stable sort of the keys
        for k, lv in enumerate(tree["levels"]):
            assert so.same(bvh.boxes.numpy()[bvh.node_ptr_host[k, b]:bvh.node_ptr_host[k, b + 1]], lv)
    assert bvh.boxes.shape[0] == bvh.level_nodes.sum() and not bvh.flags.any()


def test_too_many_faces_are_refused_before_anything_is_launched(ops):
    mesh = spatial.MeshBatch("t", [torch.zeros(3, 3, dtype=torch.float64)], [torch.zeros(2, 3, dtype=torch.int64)])
    mesh.nf = np.array([spatial.MAX_FACES + 1])
    with pytest.raises(ValueError, match="at most 16777216"):
        spatial.MeshBVH(mesh)
    assert ops.calls == []


# ------------------------------------------------------------------------------------------------------------------------- queries
def test_queries_per_mesh_equal_the_brute_force(ops):
    case = sc.ragged_case()
    bvh = spatial.build(*meshes_of(case))
    ops.calls.clear()
    t, face, point, visits = spatial.cast_rays(bvh, case["origins"], case["dirs"], case["ray_ptr"], orientation=1, return_visits=True)
    near = spatial.closest_points(bvh, case["points"], return_visits=True)
    segs = [sc.segments_of(case, b) for b in range(len(case["meshes"]))]
    a, e, skip, t_max = (np.concatenate([s[k] for s in segs], 0) for k in range(4))
    blocked, seg_visits = spatial.segments_blocked(bvh, a, e, case["ray_ptr"], skip_vertex=skip, t_max=t_max, return_visits=True)
    unlimited = spatial.segments_blocked(bvh, a, e, case["ray_ptr"])
    assert ops.calls == ["bvh_ray_cast", "bvh_closest", "bvh_blocked", "bvh_blocked"]
    for b, (v, f) in enumerate(case["meshes"]):
        rs = slice(case["ray_ptr"][b], case["ray_ptr"][b + 1])
        want = so.brute_cast(case["origins"][rs], case["dirs"][rs], v, f, 1)
        assert so.same(t[b].numpy(), want["t"]) and so.same(face[b].numpy(), want["face"]) and so.same(point[b].numpy(), want["point"])
        want = so.brute_closest(case["points"][b], v, f)
        assert all(so.same(near[b][i].numpy(), want[k]) for i, k in enumerate(("face", "bary", "distance")))
        assert len(visits[b]) == rs.stop - rs.start and len(near[b][3]) == len(case["points"][b]) and len(seg_visits[b]) == len(segs[b][0])
        assert so.same(blocked[b].numpy(), so.brute_blocked(*segs[b][:2], v, f, skip_vertex=segs[b][2], t_max=segs[b][3])["blocked"])
        assert so.same(unlimited[b].numpy(), so.brute_blocked(*segs[b][:2], v, f)["blocked"])


def test_refit_keeps_the_order_and_equals_the_brute_force_on_the_moved_mesh(ops):
    case = sc.sized_cases()[4]                                                          # 65 faces
    (v, f), = case["meshes"]
    bvh = spatial.build([v], [f])
    moved = v * np.array([1.0, -2.0, 0.5]) + 0.25
    ops.calls.clear()
    again = bvh.refit([moved])
    assert ops.calls == ["bvh_boxes"] and again.order is bvh.order and not so.same(again.boxes.numpy(), bvh.boxes.numpy())
    got = spatial.closest_points(again, [case["points"][0]])[0]
    want = so.brute_closest(case["points"][0], moved, f)
    assert all(so.same(got[i].numpy(), want[k]) for i, k in enumerate(("face", "bary", "distance")))
    assert so.same(spatial.closest_points(bvh, [case["points"][0]])[0][2].numpy(), so.brute_closest(case["points"][0], v, f)["distance"])
    with pytest.raises(ValueError, match="vertex counts"):
        bvh.refit([moved[:-1]])


def test_refusals_and_the_status_word(ops):
    case = sc.bad_face_case()
    bvh = spatial.build(*meshes_of(case))
    assert bvh.flags.tolist() == [0, ops.BVH_BAD_FACE, 0]
    with pytest.raises(ValueError, match="outside its mesh"):
        spatial.cast_rays(bvh, case["origins"], case["dirs"], case["ray_ptr"])
    with pytest.raises(ValueError, match="outside its mesh"):
        spatial.closest_points(bvh, case["points"])
    good = spatial.build(*meshes_of(sc.sized_cases()[2]))
    with pytest.raises(ValueError, match="orientation"):
        spatial.cast_rays(good, np.zeros((1, 3)), np.ones((1, 3)), [0, 1], orientation=2)
    with pytest.raises(ValueError, match="one segment per mesh"):
        spatial.cast_rays(good, np.zeros((1, 3)), np.ones((1, 3)), [0, 1, 1])
    with pytest.raises(ValueError, match="one integer per segment"):
        spatial.segments_blocked(good, np.zeros((2, 3)), np.ones((2, 3)), [0, 2], skip_vertex=[0.5, 1.0])
    with pytest.raises(ValueError, match="one value per segment"):
        spatial.segments_blocked(good, np.zeros((2, 3)), np.ones((2, 3)), [0, 2], t_max=[1.0])
    with pytest.raises(ValueError, match="outside its mesh"):
        spatial.segments_blocked(bvh, case["origins"], case["origins"] + case["dirs"], case["ray_ptr"])
    with pytest.raises(ValueError, match="one point set per mesh"):
        spatial.closest_points(good, [np.zeros((1, 3)), np.zeros((1, 3))])
    assert spatial.closest_points(spatial.build([], []), []) == []


# ------------------------------------------------------------------------------------------------------------------------- accel routes
def same_tensors(a, b):
    return all(so.same(x.numpy(), y.numpy()) for x, y in zip(a, b))


def test_cast_rays_routes_through_the_tree_only_on_request(ops):
    case = sc.ragged_case()
    verts, faces = meshes_of(case)
    plain = labels.cast_rays(case["origins"], case["dirs"], case["ray_ptr"], verts, faces, orientation=-1)
    assert ops.calls == ["ray_cast"]
    ops.calls.clear()
    tree = labels.cast_rays(case["origins"], case["dirs"], case["ray_ptr"], verts, faces, orientation=-1, accel="bvh")
    assert ops.calls == ["mesh_bbox", "bvh_build_keys", "bvh_boxes", "bvh_ray_cast"]
    assert all(same_tensors(a, b) for a, b in zip(plain, tree))
    with pytest.raises(ValueError, match="accel"):
        labels.cast_rays(case["origins"], case["dirs"], case["ray_ptr"], verts, faces, accel="kd")
    bad = sc.bad_face_case()
    with pytest.raises(ValueError, match="outside its mesh"):
        labels.cast_rays(bad["origins"], bad["dirs"], bad["ray_ptr"], *meshes_of(bad), accel="bvh")


def test_bone_ray_labels_route(ops):
    v, f, pos, hier = lo.generated_scene(16)
    rig = SimpleNamespace(pos=pos, hierarchy=hier)
    plain = labels.bone_ray_labels([v], [f], [rig])
    assert ops.calls == ["ray_cast", "ray_select", "ray_attention"]
    ops.calls.clear()
    tree = labels.bone_ray_labels([v], [f], [rig], accel="bvh")
    assert ops.calls == ["mesh_bbox", "bvh_build_keys", "bvh_boxes", "bvh_ray_cast", "ray_select", "ray_attention"]
    assert so.same(plain[0][0].numpy(), tree[0][0].numpy()) and so.same(plain[0][1].numpy(), tree[0][1].numpy())
    assert all(so.same(plain[0][2][k].numpy(), tree[0][2][k].numpy()) for k in plain[0][2])


def test_transfer_routes_through_the_tree_only_on_request(ops):
    case = sc.ragged_case()
    verts, faces = meshes_of(case)
    skins = [to.random_skins(len(v), 3 + b % 2, b) for b, v in enumerate(verts)]
    plain = transfer.transfer_skins(verts, faces, skins, case["points"])
    assert ops.calls == ["transfer_closest", "transfer_rows"]
    ops.calls.clear()
    tree = transfer.transfer_skins(verts, faces, skins, case["points"], accel="bvh")
    assert ops.calls == ["mesh_bbox", "bvh_build_keys", "bvh_boxes", "bvh_closest", "transfer_rows"]
    assert all(same_tensors(a, b) for a, b in zip(plain, tree))
    with pytest.raises(ValueError, match="accel"):
        transfer.transfer_skins(verts, faces, skins, case["points"], accel=True)
    rigs = [SimpleNamespace(skins=s) for s in skins]
    with pytest.raises(ValueError, match="without faces"):                              # MORIG_TRANSFER_NO_FACES reaches transfer_rigs
        transfer.transfer_rigs(rigs, list(zip(verts, faces)), case["points"], accel="bvh")
    keep = [0, 2, 3, 6]
    out = transfer.transfer_rigs([rigs[b] for b in keep], [(verts[b], faces[b]) for b in keep], [case["points"][b] for b in keep], accel="bvh")
    assert all(so.same(out[i].skins, plain[b][0].numpy()) for i, b in enumerate(keep))
