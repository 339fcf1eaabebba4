"""CPU: the two visibility rules on the mesh BVH without a device.

The oracle (tests/visibility_oracle.py): on every case of tests/visibility_cases.py its tree walk equals its brute force with NO query
excused; the restated brute force equals scan_oracle.visibility on that oracle's firm vertices and skin_oracle.ray_caster on its sure
rays; the amount of pruning. The host side: csrc/bonevis_core.h and the padded entering rule as the stand-alone program
tools/visibility_host_check.cpp under the address and undefined-behaviour sanitizers; the C ABI's refusals; the routes on the emulated
op layers (tests/visibility_emulate.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import scan_oracle as sco
import skin_oracle as sko
import spatial_oracle as so
import visibility_cases as vc
import visibility_emulate as ve
import visibility_oracle as vo
from morig_amd import abi, geodesic, native, runtime, scan, spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = {c["name"]: c for c in vc.scan_cases() + [vc.scan_bad_face_case()]}
BONE = {c["name"]: c for c in vc.bone_cases()}


@functools.lru_cache(maxsize=None)
def scan_results(name):
    """per view (brute, walk) of a scan case, the faces of every mesh ordered on its first view: computed once, never modified"""
    c = SCAN[name]
    orders, out = {}, []
    for v, m, cam in c["views"]:
        if m not in orders:
            orders[m] = vo.mesh_order(v, so.clamped(v, c["faces"][m])[0])
        cm = vc.camera_of(cam)
        args = (cm.row(), cm.kind, cm.width, cm.height, c["vis_eps"])
        out.append((vo.brute_scan(v, c["faces"][m], *args), vo.walk_scan(vo.view_tree(v, c["faces"][m], orders[m]), *args)))
    return out


@functools.lru_cache(maxsize=None)
def bone_results(name):
    return [(vo.brute_bone(p, b, t, f), vo.walk_bone(so.build(t, f), p, b)) for p, b, t, f in BONE[name]["meshes"]]


# ------------------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", list(SCAN))
def test_the_scan_walk_equals_the_brute_force_with_nothing_excused(name):
    for k, (brute, walk) in enumerate(scan_results(name)):
        assert so.same(walk["vis"], brute["vis"]) and walk["bad"] == brute["bad"] == (name == "bad_face"), (name, k)
        assert not walk["visits"][~brute["seen"]].any()                                 # outside the frustum nothing is walked


@pytest.mark.parametrize("name", list(BONE))
def test_the_bone_walk_equals_the_brute_force_with_nothing_excused(name):
    for k, (brute, walk) in enumerate(bone_results(name)):
        assert so.same(walk["vis"], brute["vis"]) and not walk["bad"] and not brute["bad"], (name, k)


def test_the_cases_cover_what_they_claim():
    assert {len(c["faces"][0]) for c in vc.scan_sized_cases()} >= set(vc.SCAN_FACE_COUNTS)
    assert {len(c["views"][0][0]) for c in vc.scan_sized_cases()} >= set(vc.SCAN_VERTEX_COUNTS)
    assert [m for _, m, _ in vc.scan_batch_case()["views"]] == [1, 0, 1] and len(vc.scan_batch_case()["faces"]) == 3
    assert [len(c["meshes"][0][3]) for c in vc.bone_sized_cases()] == list(vc.BONE_FACE_COUNTS)
    assert {len(m[1]) for c in vc.bone_cases() for m in c["meshes"]} >= {1, 2, 5, 33}
    for eps, want in vc.STRICT_WANT.items():                                            # strictness, decided exactly
        (brute, _), = scan_results(f"strict_eps{eps}")
        assert tuple(brute["vis"][:5]) == want, eps
    (brute, walk), = scan_results("outside_the_frustum")[:1]
    assert 0 < brute["seen"].sum() < len(brute["seen"]) and walk["visits"][brute["seen"]].all()
    assert not scan_results("outside_the_frustum")[1][0]["seen"].all()
    (brute, _), = bone_results("boxed_in")
    col = brute["vis"].reshape(-1, 2)
    assert not col[:3, 0].any() and col[:2, 1].all()                                    # the boxed-in bone sees nothing outside its cube
    assert not col[2, 1]                                                                # and the cube lies between the free bone and this vertex
    p, b, t, f = BONE["occluder_257"]["meshes"][0]
    assert vo.bone_rays(p, b)[2][0] == 0.0                                              # a ray of length zero
    assert (np.abs(b[:, 3:6] - b[:, 0:3]).sum(1) == 0).any() or len(b) < 7
    (brute, _), = bone_results("rays_in_a_plane")
    assert brute["vis"].reshape(-1, 3)[:4, 0].all()                                     # det == 0: the plane's own faces are never hit
    (brute, _), = bone_results("no_occluder_vertices")
    assert brute["vis"].all()


def test_the_restated_scan_rule_equals_the_scan_oracle_on_its_firm_vertices():
    for c in vc.scan_generated_cases() + vc.scan_torus_cases()[:2]:
        (v, m, cam), = c["views"]
        cm = vc.camera_of(cam)
        want, firm = sco.visibility(v, c["faces"][m], cm.row(), cm.kind, cm.width, cm.height, c["vis_eps"])
        (brute, _), = scan_results(c["name"])
        assert firm.mean() > 0.99 and np.array_equal(brute["vis"][firm], want[firm]), c["name"]


def test_the_restated_bone_rule_equals_the_skin_oracle_on_its_sure_rays():
    for name in ("torus_own_occluder", "occluder_4097", "occluder_1922", "occluder_257"):
        (p, b, t, f), = BONE[name]["meshes"]
        want, unsure, _ = sko.bone_visibility(p, b, t, f)
        share = unsure.mean()
        print(f"{name}: {unsure.sum()} of {unsure.size} rays unsure ({100 * share:.3f} %)")
        (brute, _), = bone_results(name)
        sure = ~unsure.reshape(-1)
        assert np.array_equal(brute["vis"][sure] != 0, want.reshape(-1)[sure]), name
        if name == "torus_own_occluder":
            assert share <= 1e-3                                                        # what the existing differential test allows


def test_pruning_stays_under_its_caps():
    for kind in ("orthographic", "pinhole"):
        (_, walk), = scan_results(f"torus_4096_{kind}")
        share = walk["visits"].sum() / (len(walk["visits"]) * 4096)
        print(f"scan {kind}: {share:.4f} of Q x F (cap {vc.SCAN_CAP[kind]})")
        assert 0 < share < vc.SCAN_CAP[kind]
    (_, fresh), (_, stale) = scan_results("torus_4096_stale")
    share = stale["visits"].sum() / (len(stale["visits"]) * 4096)
    print(f"scan, rest order on the bent pose: {share:.4f} of Q x F (cap {vc.STALE_CAP})")
    assert 0 < share < vc.STALE_CAP
    (_, walk), = bone_results("torus_own_occluder")
    share = walk["visits"].sum() / (len(walk["visits"]) * len(BONE["torus_own_occluder"]["meshes"][0][3]))
    print(f"bone: {share:.4f} of Q x F (cap {vc.BONE_CAP})")
    assert 0 < share < vc.BONE_CAP


def test_a_stale_order_gives_the_fresh_orders_mask():
    c = SCAN["torus_4096_stale"]
    v, m, cam = c["views"][1]
    cm = vc.camera_of(cam)
    fresh = vo.walk_scan(vo.view_tree(v, c["faces"][m], vo.mesh_order(v, c["faces"][m])), cm.row(), cm.kind, cm.width, cm.height, c["vis_eps"])
    stale = scan_results("torus_4096_stale")[1][1]
    print(f"bent pose: {fresh['visits'].sum() / (len(v) * 4096):.4f} of Q x F in its own order, {stale['visits'].sum() / (len(v) * 4096):.4f} in the rest pose's")
    assert so.same(fresh["vis"], stale["vis"])


def test_every_accepted_face_is_entered_from_the_root_down():
    """the equality arguments of DESIGN.md section 28 on the generated scenes: the box of an accepted face and every box above it passes
    the entering rule, with the bound 1 for the scan rule and with the face's own t as the best for the bone rule"""
    c = SCAN["torus_4096_pinhole"]
    (v, m, cam), = c["views"]
    cm = vc.camera_of(cam)
    tree = vo.view_tree(v, c["faces"][m], vo.mesh_order(v, c["faces"][m]))
    o, d, ln, seen = vo.scan_rays(v, cm.row(), cm.kind, cm.width, cm.height)
    tri = tree["verts"][tree["faces"][tree["order"]]]
    n = 0
    for q in np.flatnonzero(seen)[::16]:
        hit, _ = vo._blocks(o[q][None], d[q][None], ln[q], c["vis_eps"], tri[:, 0], tri[:, 1], tri[:, 2])
        scale = so.query_scale(o[q], tree["levels"][-1][0])
        for at in np.flatnonzero(hit):
            n += 1
            assert vo.entered_above(tree, at, lambda boxes: vo.ray_skips(o[q], d[q], boxes, scale, 1.0))
    (p, b, t, f), = BONE["torus_own_occluder"]["meshes"]
    tree = so.build(t, f)
    tri = tree["verts"][tree["faces"][tree["order"]]]
    o, d, ln, dn = vo.bone_rays(p, b)
    for q in range(0, len(o), 8):
        ts = vo.bone_hits(o[q], d[q], dn[q], tri[:, 0], tri[:, 1], tri[:, 2])
        scale = so.query_scale(o[q], tree["levels"][-1][0])
        for at in np.flatnonzero(ts < np.inf):
            n += 1
            assert vo.entered_above(tree, at, lambda boxes: vo.ray_skips(o[q], d[q], boxes, scale, ts[at], vo.BONE_SLACK))
    assert n > 1000


def test_the_padded_entering_rule_defaults_to_the_existing_one():
    rng = np.random.default_rng(5)
    lo_, ext = rng.normal(size=(200, 3)), rng.uniform(0, 1, (200, 3))
    boxes = np.concatenate([lo_, lo_ + ext], 1)
    for k in range(20):
        o, d = rng.normal(size=3) * 3, rng.normal(size=3) * (rng.uniform(size=3) < 0.8)
        a, b = so.ray_skips(o, d, boxes, 7.0, 2.5), vo.ray_skips(o, d, boxes, 7.0, 2.5)
        assert so.same(a[0], b[0]) and so.same(a[1], b[1])
        wide = vo.ray_skips(o, d, boxes, 7.0, 2.5, vo.BONE_SLACK)
        assert not (wide[0] & ~a[0]).any()                                              # a larger pad never skips more


# ------------------------------------------------------------------------------------------------------------------------- the host side
def test_the_rule_headers_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "visibility_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "visibility_host_check.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "" and done.stdout.strip().endswith("ok"), (done.returncode, done.stdout[-2000:], done.stderr[-2000:])


def test_the_abi_has_the_three_entry_points_and_refuses_without_a_device():
    names = ["morig_bvh_view_boxes", "morig_bvh_scan_visibility", "morig_bvh_bone_visibility"]
    assert set(names) <= set(native.EXPORTS) and len(abi.STRUCTS) == 8                 # plain parameters: no new argument struct
    lib, K = native.load_library(), abi.CONSTANTS
    none4, none6 = (None,) * 4, (None,) * 6
    assert lib.morig_bvh_view_boxes(None, None, None, 1, None, None, 1, 64 ** 4 + 1, None, None, 1, 0, 0, 0, None, None, None) == K["MORIG_E_UNSUPPORTED"]
    assert lib.morig_bvh_view_boxes(None, None, None, -1, None, None, 1, 10, None, None, 1, 0, 0, 0, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_bvh_view_boxes(None, None, None, 1, None, None, 1, 10, None, None, 1, 0, 0, 0, None, None, None) == K["MORIG_E_INVALID"]   # no flag words
    assert lib.morig_bvh_view_boxes(None, None, None, 0, None, None, 0, 0, None, None, 0, 0, 0, 0, None, None, None) == K["MORIG_OK"]          # no view
    assert lib.morig_bvh_scan_visibility(*none6, 1, 1, 4, 0.0, *none4, None, None, None, None) == K["MORIG_E_INVALID"]                         # no status word
    assert lib.morig_bvh_scan_visibility(*none6, 1, 1, -1, 0.0, *none4, None, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_bvh_bone_visibility(*none6, None, None, None, 1, 4, *none4, None, None, None, None) == K["MORIG_E_INVALID"]               # no status word
    assert lib.morig_bvh_bone_visibility(*none6, None, None, None, 1, -1, *none4, None, None, None, None) == K["MORIG_E_INVALID"]


@pytest.fixture
def ops():
    emu = ve.VisibilityOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def _scan_inputs(c):
    return [v for v, _, _ in c["views"]], c["faces"], [vc.camera_of(cam) for _, _, cam in c["views"]], [m for _, m, _ in c["views"]]


def test_scan_routes_launch_what_they_launched_and_the_tree_with_accel(ops):
    c = vc.scan_batch_case()
    verts, faces, cams, view_mesh = _scan_inputs(c)
    plain = scan.scan_meshes(verts, faces, cams, corr_radius=0.05, view_mesh=view_mesh)
    before = list(ops.calls)
    assert before == ["scan_raster", "scan_resolve", "scan_compact", "scan_visibility", "scan_nearest", "scan_nearest"]
    del ops.calls[:]
    tree = scan.scan_meshes(verts, faces, cams, corr_radius=0.05, view_mesh=view_mesh, accel="bvh")
    assert ops.calls == ["scan_raster", "scan_resolve", "scan_compact", "mesh_bbox", "bvh_build_keys", "bvh_view_boxes", "bvh_scan_visibility",
                         "scan_nearest", "scan_nearest"]
    for a, b in zip(plain, tree):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    del ops.calls[:]
    chunked = scan.scan_meshes(verts, faces, cams, corr_radius=0.05, view_mesh=view_mesh, accel="bvh", key_budget=1)
    assert ops.calls.count("bvh_build_keys") == 1 and ops.calls.count("bvh_view_boxes") == 3      # one order per job, boxes per chunk
    for a, b in zip(plain, chunked):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match='accel is None or "bvh"'):
        scan.scan_meshes(verts, faces, cams, view_mesh=view_mesh, accel="kd")
    with pytest.raises(ValueError, match='accel is None or "bvh"'):
        scan.scan_trajectory([np.zeros((3, 2, 3))], [np.zeros((0, 3), dtype=np.int64)], [cams[0]], n_pts=1, accel=True)


def test_scan_trajectory_passes_accel_on_and_a_bad_face_stays_a_value_error(ops):
    c = vc.scan_sized_cases()[2]
    (v, _, cam), = c["views"]
    traj = np.stack([v, vc.bent(v, 20.0)], 1)
    cm = vc.camera_of(cam)
    n = int((sco.render(v, c["faces"][0], cm.row(), cm.kind, cm.width, cm.height)["face"] >= 0).sum())
    plain = scan.scan_trajectory([traj], c["faces"], [cm], n_pts=min(n, 8), corr_radius=0.05)
    del ops.calls[:]
    tree = scan.scan_trajectory([traj], c["faces"], [cm], n_pts=min(n, 8), corr_radius=0.05, accel="bvh")
    assert "bvh_scan_visibility" in ops.calls and "scan_visibility" not in ops.calls
    assert all(torch.equal(x, y) for x, y in zip(plain[0], tree[0]))
    bad = vc.scan_bad_face_case()
    verts, faces, cams, view_mesh = _scan_inputs(bad)
    for accel in (None, "bvh"):
        with pytest.raises(ValueError, match="outside its mesh"):
            scan.scan_meshes(verts, faces, cams, view_mesh=view_mesh, accel=accel)


def test_build_views_orders_once_per_mesh_and_boxes_every_view(ops):
    c = vc.scan_batch_case()
    verts, faces, _, view_mesh = _scan_inputs(c)
    tree = spatial.build_views(verts, faces, view_mesh)
    assert ops.calls == ["mesh_bbox", "bvh_build_keys", "bvh_view_boxes"]
    fp = np.concatenate([[0], np.cumsum([len(f) for f in faces])])
    for m, first in ((1, 0), (0, 1)):
        assert np.array_equal(tree.order.numpy()[fp[m]:fp[m + 1]] - fp[m], vo.mesh_order(verts[first], faces[m]))
    for v, m in enumerate(view_mesh):
        want = vo.view_tree(verts[v], faces[m], tree.order.numpy()[fp[m]:fp[m + 1]] - fp[m])
        for k, lv in enumerate(want["levels"]):
            assert so.same(tree.boxes.numpy()[tree.node_ptr_host[k, v]:tree.node_ptr_host[k, v + 1]], lv)
    assert tree.boxes.shape[0] == tree.level_nodes.sum() and not tree.flags.any()
    with pytest.raises(ValueError, match="view_mesh names one mesh"):
        spatial.build_views(verts, faces, [0, 1, 3])


def test_bone_routes_launch_what_they_launched_and_the_tree_with_accel(ops):
    c = vc.bone_ragged_cases()[0]
    ms = c["meshes"][:2] + c["meshes"][3:]
    cols = [[m[k] for m in ms] for k in range(4)]
    plain = geodesic.bone_visibility_batched(*cols)
    assert ops.calls == ["bone_visibility"]
    del ops.calls[:]
    tree = geodesic.bone_visibility_batched(*cols, accel="bvh")
    assert ops.calls == ["mesh_bbox", "bvh_build_keys", "bvh_boxes", "bvh_bone_visibility"]
    assert all(a.dtype == torch.bool and torch.equal(a, b) for a, b in zip(plain, tree))
    one = geodesic.bone_visibility(*ms[0], accel="bvh")
    assert torch.equal(one, plain[0])
    with pytest.raises(ValueError, match='accel is None or "bvh"'):
        geodesic.bone_visibility(*ms[0], accel="octree")
    with pytest.raises(ValueError, match="out of range"):
        geodesic.bone_visibility(ms[0][0], ms[0][1], ms[0][2], ms[0][3] + len(ms[0][2]), accel="bvh")
