"""CPU: the oracle of the non-manifold split (tests/manifold_oracle.py) on answers known by hand; the host logic of
``morig_amd.meshprep.split_nonmanifold`` / ``repair(split=True)`` / ``prepare_mesh(split=True)`` on an emulated op layer
(tests/manifold_emulate.py through ``runtime._test_ops``) against that oracle; the new exports' typing and refusals through the C ABI; and
csrc/fan_core.h as the stand-alone program tools/manifold_host_check.cpp, built with the address and undefined-behaviour sanitizers and
run as a program (never loaded into Python)."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import manifold_emulate as me
import manifold_oracle as mo
import repair_emulate as re_
import repair_oracle as ro
import topology_oracle as to
from morig_amd import abi, meshprep, native, runtime
from test_repair_oracle import same_result as same_repaired

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops():
    emu = me.ManifoldOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def cases():
    """(name, mesh, orientable): the cases of the issue's table"""
    return [("fan5", to.fan(5), True), ("fan200", to.fan(200, flip=(3, 77, 199)), True), ("tetrahedra", to.shared_edge_tetrahedra(), True),
            ("bowtie", ro.bowtie(), True), ("touching", ro.cube_two_holes_touching(), True), ("cones2", mo.cones(2), True),
            ("cones65", mo.cones(65, apex="random", seed=3), True), ("pinched_torus", mo.pinched_torus(), True), ("fin", mo.cube_with_fin(), True),
            ("corner_cubes", mo.cubes_at_a_corner(), True), ("moebius", to.mobius(), False), ("cube", ro.cube(), True), ("torus", to.torus(6, 5), True),
            ("strip", to.strip(12), True)]


# ------------------------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("name,mesh,orientable", cases(), ids=[c[0] for c in cases()])
def test_every_line_of_the_table(name, mesh, orientable):
    v, f = mesh
    s = mo.split(v, f)
    cv, cf, _, _ = to.clean(v, f)
    # the faces, their order and their corners are unchanged; nothing moves; no edge keeps three faces (the chain-end property)
    assert np.array_equal(s["source"][s["faces"]], cf) and s["verts"].tobytes() == cv[s["source"]].tobytes()
    assert np.array_equal(s["source"][:len(cv)], np.arange(len(cv))) and len(s["verts"]) == len(cv) + s["report"]["added_verts"]
    after = to.diagnose(s["verts"], s["faces"], weld=False)
    assert after["nonmanifold_edges"] == 0 and after["faces"] == len(cf)
    # a second application with the weld off adds nothing and returns the same faces
    again = mo.split(s["verts"], s["faces"], weld=False)
    assert again["report"]["added_verts"] == 0 and np.array_equal(again["faces"], s["faces"]) and again["verts"].tobytes() == s["verts"].tobytes()
    assert np.array_equal(again["vertex_map"], np.arange(len(s["verts"]))) and np.array_equal(again["face_map"], np.arange(len(s["faces"])))
    # the re-weld trap: the default weld joins the copies again
    if s["report"]["added_verts"]:
        back = to.diagnose(s["verts"], s["faces"])
        assert back["duplicate_verts"] == s["report"]["added_verts"] and back["nonmanifold_edges"] == s["report"]["nonmanifold_edges"]
    r = ro.repair(s["verts"], s["faces"], weld=False, fill_holes="all")
    if orientable:
        assert r["report"]["tangled_boundary_edges"] == 0 and r["report"]["nonorientable_components"] == 0
        assert to.diagnose(r["verts"], r["faces"], weld=False)["watertight"]
    else:
        assert r["report"]["nonorientable_components"] == 1 and r["report"]["tangled_boundary_edges"] > 0
        assert s["report"]["added_verts"] == 0 and np.array_equal(s["faces"], f) and s["verts"].tobytes() == v.tobytes()


def test_bowtie_and_touching_holes_become_one_simple_loop_each():
    for mesh, tangled, length in ((ro.bowtie(), 16, 16), (ro.cube_two_holes_touching(), 6, 6)):
        before = ro.repair(*mesh, fill_holes="all")["report"]
        assert (before["tangled_boundary_edges"], before["boundary_loops"], before["filled_loops"]) == (tangled, 0, 0)
        r = mo.repair_split(*mesh, fill_holes="all")
        assert (r["report"]["tangled_boundary_edges"], r["report"]["boundary_loops"], r["report"]["filled_loops"]) == (0, 1, 1)
        assert list(map(len, r["loops"].values())) == [length] and r["report"]["split"]["added_verts"] == 1
        assert r["report"]["split"]["nonmanifold_verts"] == 1 and r["report"]["split"]["nonmanifold_edges"] == 0 and r["source"][-1] == -1


def test_shared_edge_tetrahedra_come_apart_into_two_closed_components():
    v, f = to.shared_edge_tetrahedra()
    s = mo.split(v, f)
    assert s["report"]["nonmanifold_edges"] == 1 and s["report"]["added_verts"] == 2 and s["source"][-2:].tolist() == [0, 1]
    assert np.array_equal(s["faces"][:4], f[:4]) and sorted(set(s["faces"][4:].reshape(-1).tolist())) == [4, 5, 6, 7]
    d = to.diagnose(s["verts"], s["faces"], weld=False)
    assert d["watertight"] and d["components"] == 2 and d["euler"] == 4
    # closed now: each is judged by its volume, so the second comes out the same way whichever way it went in
    ra, rb = mo.repair_split(v, f), mo.repair_split(v, ro.flip_faces(f, [4, 5, 6, 7]))
    assert ra["report"]["closed_components"] == rb["report"]["closed_components"] == 2 and ro.repair(v, f)["report"]["closed_components"] == 0
    assert np.array_equal(ra["faces"], rb["faces"]) and (ra["report"]["inverted_components"], rb["report"]["inverted_components"]) == (2, 1)
    assert ra["flipped"].all() and rb["flipped"][:4].all() and not rb["flipped"][4:].any()     # the generator winds both inward
    assert all(x > 0 for x in ro.orientation(ra["verts"], ra["faces"])["volume"].values())


@pytest.mark.parametrize("k", [2, 3, 5, 64])
def test_k_faces_on_one_edge_give_k_components(k):
    v, f = to.fan(k, flip=(1,))
    s = mo.split(v, f)
    rep = s["report"]
    assert (rep["added_verts"], rep["max_fans"], rep["nonmanifold_verts"], rep["fans"]) == (2 * (k - 1) if k > 2 else 0, k if k > 2 else 1, 2 if k > 2 else 0,
                                                                                        3 * k if k > 2 else 4)
    assert to.diagnose(s["verts"], s["faces"], weld=False)["components"] == (k if k > 2 else 1) and rep["nonmanifold_edges"] == int(k > 2)


def test_cones_fin_pinch_and_corner_by_hand():
    s = mo.split(*mo.cones(65))
    assert (s["report"]["added_verts"], s["report"]["max_fans"], s["report"]["nonmanifold_verts"], s["report"]["nonmanifold_edges"]) == (64, 65, 1, 0)
    assert (s["source"][-64:] == 0).all() and to.diagnose(s["verts"], s["faces"], weld=False)["components"] == 65
    s = mo.split(*mo.cube_with_fin())
    assert (s["report"]["nonmanifold_edges"], s["report"]["added_verts"], s["report"]["nonmanifold_verts"]) == (1, 2, 2)
    assert np.array_equal(s["faces"][:12], ro.cube()[1]) and s["faces"][12].tolist() == [9, 10, 8]     # the cube keeps its vertices, the fin gets copies
    s = mo.split(*mo.pinched_torus())
    assert (s["report"]["nonmanifold_edges"], s["report"]["added_verts"], s["report"]["max_fans"]) == (0, 1, 2)
    d = to.diagnose(s["verts"], s["faces"], weld=False)
    assert d["watertight"] and d["euler"] == 0 and d["components"] == 1
    s = mo.split(*mo.cubes_at_a_corner())
    d = to.diagnose(s["verts"], s["faces"], weld=False)
    assert s["report"]["added_verts"] == 1 and d["components"] == 2 and d["watertight"] and s["report"]["input"]["duplicate_verts"] == 1
    v, f = mo.folded_bowtie_box()
    assert to.diagnose(v, f)["boundary_edges"] == 8 and ro.repair(v, f, fill_holes="all")["report"]["tangled_boundary_edges"] == 8
    r = mo.repair_split(v, f, fill_holes="all")
    assert r["report"]["filled_loops"] == 1 and to.diagnose(r["verts"], r["faces"], weld=False)["watertight"]


def test_the_round_count_is_that_of_the_component_rule_on_the_corner_links():
    v, f = mo.disc(1025)
    cf = to.clean(v, f)[1]
    pairs, _ = mo.corner_links(cf)
    assert mo.split(v, f)["report"]["split_rounds"] == to.cc_rounds(3 * len(cf), pairs)[1] >= 3
    assert mo.split(*to.strip(3))["report"]["split_rounds"] == 1                 # one face: nothing links, the verifying round alone


def test_padding_puts_the_runs_where_the_kernels_change_blocks():
    cf = to.clean(*mo.padded(to.fan(2, flip=(1,)), 85))[1]                       # 255 records of padding: the one two-run sits at 255 / 256
    assert mo.run_at(cf, 255, 256) == (255, 2)
    cf = to.clean(*mo.padded(to.fan(200, flip=(5, 150)), 52))[1]                 # the run of 200 begins at 156 and crosses 256
    at, n = mo.run_at(cf, 156, 157)
    assert n == 200 and at < 256 < at + n
    cf = to.clean(*mo.padded(mo.disc(6, closed=True), 84))[1]                    # faces 84 ..: the centre's corners are nodes 252, 255, 258, ...
    assert [3 * i + list(t).index(252) for i, t in enumerate(cf) if 252 in t] == [252, 255, 258, 261, 264, 267]


# ------------------------------------------------------------------------------------------------------------------------- host logic
def batch_cases():
    rng = np.random.default_rng(5)
    cv, cf = ro.cube()
    out = [(n, m) for n, m, _ in cases() if n != "fan200"]
    tv, tf = mo.pinched_torus()
    nan = mo.cones(3)[0].copy()
    nan[0] = [np.nan, -0.0, 1.0]
    out += [("fan9", to.fan(9, flip=(2, 5))), ("torus_flipped", (tv, ro.flip_faces(tf, rng.choice(len(tf), 18, replace=False)))),
            ("disc_path", mo.disc(65, centre="random", seed=1)), ("disc_cycle", mo.disc(64, closed=True, centre="highest")),
            ("nan_apex", (nan, mo.cones(3)[1])), ("box", mo.folded_bowtie_box()),
            ("raw", (np.concatenate([mo.cube_with_fin()[0], cv[:2], [[9.0, 9, 9]]]),
                     np.concatenate([mo.cube_with_fin()[1], [[9, 10, 3], [0, 0, 1], cf[5][[1, 2, 0]]]]))),
            ("no_faces", (cv, np.zeros((0, 3), dtype=np.int64)))]
    return out


def same_split(got, want, report=None):
    v, f, vm, fm, src = got
    assert v.dtype == torch.float64 and f.dtype == vm.dtype == fm.dtype == src.dtype == torch.int64
    assert v.cpu().numpy().tobytes() == want["verts"].tobytes() and tuple(v.shape) == want["verts"].shape
    for x, k in ((f, "faces"), (vm, "vertex_map"), (fm, "face_map"), (src, "source")):
        assert np.array_equal(x.cpu().numpy(), want[k]) and tuple(x.shape) == want[k].shape, k
    if report is not None:
        for k in mo.FIELDS + ("split_rounds",):
            assert report[k] == want["report"][k] and type(report[k]) is int, (k, report[k], want["report"][k])
        for k in to.FIELDS:
            assert report["input"][k] == want["report"]["input"][k], k


def same_repair(got, want, report=None):
    assert len(got) == 6
    same_repaired(got[:5], want, report)
    assert got[5].dtype == torch.int64 and np.array_equal(got[5].cpu().numpy(), want["source"])
    if report is not None:
        assert report["split"] == want["report"]["split"] and all(type(x) is int for x in report["split"].values())


def test_split_on_the_emulated_ops_equals_the_oracle(ops):
    meshes = [m for _, m in batch_cases()]
    out, reports = meshprep.split_nonmanifold([m[0] for m in meshes], [m[1] for m in meshes], return_report=True)
    for (name, (v, f)), o, r in zip(batch_cases(), out, reports):
        print(name, {k: r[k] for k in mo.FIELDS + ("split_rounds",)})
        same_split(o, mo.split(v, f), r)
    assert tuple(reports[0])[:len(mo.FIELDS)] == meshprep.SPLIT_FIELDS == mo.FIELDS
    assert ops.calls.count("meshsplit_links") == ops.calls.count("meshsplit_fans") == ops.calls.count("meshsplit_apply") == 1
    alone = meshprep.split_nonmanifold([meshes[3][0]], [meshes[3][1]])           # a mesh alone: what it gives in the batch
    for x, y in zip(alone[0], out[3]):
        assert torch.equal(x, y)
    for keep, weld in (("largest", True), (11, True), ("all", False)):
        v, f = np.concatenate([meshes[2][0], meshes[7][0] + 5.0]), np.concatenate([meshes[2][1], meshes[7][1] + len(meshes[2][0])])
        (o,), (r,) = meshprep.split_nonmanifold([v], [f], keep=keep, weld=weld, return_report=True)
        same_split(o, mo.split(v, f, weld=weld, keep=keep), r)


def test_a_second_application_with_the_weld_off_is_the_identity(ops):
    for name, (v, f) in batch_cases():
        (a,) = meshprep.split_nonmanifold([v], [f])
        (b,), (r,) = meshprep.split_nonmanifold([a[0]], [a[1]], weld=False, return_report=True)
        assert torch.equal(b[1], a[1]) and b[0].numpy().tobytes() == a[0].numpy().tobytes() and r["added_verts"] == 0, name
        assert torch.equal(b[2], torch.arange(len(a[0]))) and torch.equal(b[3], torch.arange(len(a[1]))) and torch.equal(b[4], torch.arange(len(a[0])))
        copies = a[0].numpy()[len(to.clean(v, f)[0]):]                           # the trap: the default weld joins the copies again (a NaN never welds)
        if len(copies):
            assert meshprep.diagnose([a[0]], [a[1]])[0]["duplicate_verts"] == int(np.isfinite(copies).all(1).sum())


@pytest.mark.parametrize("orient,fill", [(True, "all"), (True, None), (False, 6)])
def test_repair_with_split_on_the_emulated_ops_equals_the_oracle(ops, orient, fill):
    meshes = [m for _, m in batch_cases()]
    out, reports = meshprep.repair([m[0] for m in meshes], [m[1] for m in meshes], orient=orient, fill_holes=fill, return_report=True, split=True)
    for (name, (v, f)), o, r in zip(batch_cases(), out, reports):
        same_repair(o, mo.repair_split(v, f, orient=orient, fill_holes=fill), r)
        if orient and fill == "all" and r["nonorientable_components"] == 0:
            assert r["tangled_boundary_edges"] == 0
            assert to.diagnose(o[0].numpy(), o[1].numpy(), weld=False)["watertight"] or len(o[1]) == 0, name
    assert ops.calls.count("meshcheck_compact") == 1 and ops.calls.count("meshfix_edge_records") == 2     # one clean; the split's records, then the repair's


def test_repair_without_split_makes_the_calls_it_made_before(ops):
    meshes = [m for _, m in batch_cases()]
    args = ([m[0] for m in meshes], [m[1] for m in meshes])
    a, ra = meshprep.repair(*args, fill_holes="all", return_report=True, split=False)
    mine = list(ops.calls)
    old = re_.RepairOps()                                                        # the op layer of the parent commit: it has no split operator
    runtime._test_ops = old
    b, rb = meshprep.repair(*args, fill_holes="all", return_report=True)
    assert mine == old.calls and not any(c.startswith("meshsplit_") for c in mine) and len(mine) > 20
    for (name, (v, f)), x, y, r, q in zip(batch_cases(), a, b, ra, rb):
        assert len(x) == len(y) == 5 and all(torch.equal(s, t) or (s.dtype == torch.float64 and s.numpy().tobytes() == t.numpy().tobytes()) for s, t in zip(x, y))
        assert list(r) == list(q) == list(ro.FIELDS) + ["orient_rounds", "input"] and "split" not in r
        same_repaired(x, ro.repair(v, f, fill_holes="all"), r)


def test_list_shapes_of_empty_inputs(ops):
    assert meshprep.split_nonmanifold([], []) == [] and meshprep.split_nonmanifold([], [], return_report=True) == ([], [])
    assert meshprep.repair([], [], split=True) == [] and not ops.calls
    e3, f3 = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    v, f = to.shared_edge_tetrahedra()
    out, reps = meshprep.split_nonmanifold([e3, v, v], [f3, f, f3], return_report=True)
    assert [tuple(o[0].shape) for o in out] == [(0, 3), (8, 3), (0, 3)] and [tuple(o[1].shape) for o in out] == [(0, 3), (8, 3), (0, 3)]
    assert [tuple(o[4].shape) for o in out] == [(0,), (8,), (0,)] and out[2][2].tolist() == [-1] * 6
    assert [r["added_verts"] for r in reps] == [0, 2, 0] and [r["split_rounds"] for r in reps] == [1, mo.split(v, f)["report"]["split_rounds"], 1]
    (only,), (r,) = meshprep.repair([e3], [f3], fill_holes="all", split=True, return_report=True)
    assert tuple(only[0].shape) == (0, 3) and tuple(only[5].shape) == (0,) and r["split"]["fans"] == 0


def test_error_texts(ops, monkeypatch):
    v, f = ro.cube()
    with pytest.raises(ValueError, match="clean: keep"):
        meshprep.split_nonmanifold([v], [f], keep="biggest")
    with pytest.raises(ValueError, match="clean: a face names a vertex outside its mesh"):
        meshprep.split_nonmanifold([v], [np.array([[0, 1, 8]])])
    with pytest.raises(ValueError, match="split_nonmanifold: weld_tol needs weld=True"):
        meshprep.split_nonmanifold([v], [f], weld=False, weld_tol=0.1)
    with pytest.raises(ValueError, match="split_nonmanifold: max_links needs a weld_tol"):
        meshprep.split_nonmanifold([v], [f], max_links=3)
    with pytest.raises(ValueError, match="prepare_mesh: split belongs to the clean / repair step"):
        meshprep.prepare_mesh(v, f, split=True)
    with pytest.raises(TypeError):
        meshprep.split_nonmanifold([v], [f], True)                               # keyword-only
    assert not ops.calls                                                         # refused before any launch
    monkeypatch.setattr(meshprep, "SPLIT_MAX_FACES", 11)
    with pytest.raises(ValueError, match="split_nonmanifold: 12 faces in one call: the split supports at most 11"):
        meshprep.split_nonmanifold([v], [f])
    assert not any(c.startswith("meshfix_") or c.startswith("meshsplit_") for c in ops.calls)     # refused before the split launches anything
    assert meshprep.SPLIT_MAX_FACES == 11 and (2 ** 31 - 257) // 6 * 6 <= 2 ** 31 - 257 < meshprep.REPAIR_MAX_FACES * 8 + 8


def test_prepare_mesh_hands_the_split_on_and_carries_source(ops, monkeypatch):
    from morig_amd import geodesic, graph_build
    seen = {}
    monkeypatch.setattr(meshprep, "normalize", lambda verts: [(torch.as_tensor(v), np.zeros(3), 1.0) for v in verts])

    def simplify(verts, faces, target_faces):
        seen["simplify"] = [tuple(v.shape) for v in verts]
        return [(v[::2], f[:1] * 0, torch.arange(len(v)) // 2, 4) for v, f in zip(verts, faces)]
    monkeypatch.setattr(meshprep, "simplify", simplify)
    monkeypatch.setattr(meshprep, "tpl_edges", lambda faces, n, self_loops: seen.update(tpl=list(n)) or [None] * len(n))
    monkeypatch.setattr(meshprep, "sample_surface", lambda v, f, **kw: seen.update(sampled=[torch.as_tensor(x) for x in f]) or ([None] * len(v), [None] * len(v)))
    monkeypatch.setattr(meshprep, "voxelize", lambda v, f, dims: [None] * len(v))
    monkeypatch.setattr(geodesic, "surface_geodesic_batched", lambda v, p, n: [None] * len(v))
    monkeypatch.setattr(graph_build, "get_geo_edges_from_distance", lambda *a: None)
    v, f = dict(batch_cases())["raw"]
    want = mo.repair_split(v, f, fill_holes="all")
    d = meshprep.prepare_mesh(v, f, repair=True, split=True)
    assert np.array_equal(d["vertex_map"].numpy(), want["vertex_map"]) and np.array_equal(d["faces"].numpy(), want["faces"])
    assert np.array_equal(d["source"].numpy(), want["source"]) and np.array_equal(d["flipped"].numpy(), want["flipped"])
    assert seen["tpl"] == [len(want["verts"])] and np.array_equal(seen["sampled"][0].numpy(), want["faces"]) and d["report"]["split"]["added_verts"] == 2
    assert ops.calls.count("meshcheck_compact") == 1 and ops.calls.count("meshsplit_apply") == 1
    d = meshprep.prepare_mesh(v, f, repair=True, split=True, simplify_to=5)
    assert seen["simplify"] == [want["verts"].shape]
    assert np.array_equal(d["vertex_map"].numpy(), np.where(want["vertex_map"] >= 0, want["vertex_map"] // 2, -1))
    ops.calls.clear()
    want = mo.split(v, f)
    d = meshprep.prepare_mesh(v, f, clean=True, split=True)
    assert np.array_equal(d["faces"].numpy(), want["faces"]) and np.array_equal(d["source"].numpy(), want["source"]) and "flipped" not in d
    assert np.array_equal(d["vertex_map"].numpy(), want["vertex_map"]) and d["report"]["added_verts"] == 2 and seen["tpl"] == [len(want["verts"])]
    assert ops.calls.count("meshcheck_compact") == 1 and not any(c.startswith("meshfix_orient") for c in ops.calls)
    ops.calls.clear()
    d = meshprep.prepare_mesh(v, f, clean=True)                                  # without the argument: no split call, no source
    assert not any(c.startswith("meshsplit_") for c in ops.calls) and "source" not in d


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_exports_are_typed_and_refuse_bad_arguments_without_a_device():
    names = [n for n in abi.SIGNATURES if n.startswith("morig_meshsplit_")]
    assert len(names) == 3 and set(names) <= set(native.EXPORTS) and len(abi.STRUCTS) == 8        # plain parameters: no new argument struct
    lib = native.load_library()
    K = abi.CONSTANTS
    for n in names:
        assert getattr(lib, n).argtypes is not None and hasattr(native.NativeOps, n[len("morig_"):])
    N = None
    calls = {                                                                     # name -> (arguments with a count of 4 everywhere, the count positions)
        "links": ([N, N, N, 4, 4, N, N, N], (3, 4)),
        "fans": ([N, N, 4, 4, N, N, N], (2, 3)),
        "apply": ([N, N, N, N, 4, N, N, N, 1, N, 4, 4, N, N, N, N], (4, 8, 10, 11)),
    }
    for name, (args, counts) in calls.items():
        fn = getattr(lib, "morig_meshsplit_" + name)
        assert len(args) == len(abi.SIGNATURES["morig_meshsplit_" + name][1]), name
        assert fn(*args) == K["MORIG_E_INVALID"], name                            # null pointers
        for at in counts:
            bad = list(args)
            bad[at] = -1
            assert fn(*bad) == K["MORIG_E_INVALID"], (name, at)                   # a negative count
        zero = list(args)
        for at in counts:
            zero[at] = 0
        assert fn(*zero) == K["MORIG_OK"], name                                   # nothing to do: before anything is launched
    assert lib.morig_meshsplit_links(N, N, N, 13, 4, N, N, N) == K["MORIG_E_INVALID"]                          # more records than 3 F
    assert lib.morig_meshsplit_fans(N, N, (2 ** 31 - 257) // 3 + 1, 4, N, N, N) == K["MORIG_E_INVALID"]        # 3 F past the row limit
    assert lib.morig_meshsplit_apply(N, N, N, N, 4, N, N, N, 1, N, 4, 3, N, N, N, N) == K["MORIG_E_INVALID"]   # fewer output rows than rows
    assert lib.morig_meshsplit_apply(N, N, N, N, 4, N, N, N, 1, N, 4, 17, N, N, N, N) == K["MORIG_E_INVALID"]  # more new rows than corners
    prof = [lib.morig_prof_name(k) for k in range(K["MORIG_PROF_KINDS"])]
    assert prof.index(b"meshsplit_links") == prof.index(b"proxweld_spread") + 1 and prof.index(b"meshsplit_apply") == prof.index(b"meshsplit_links") + 1


# ------------------------------------------------------------------------------------------------------------------------- the host program
def test_fan_core_under_the_sanitizers_equals_a_brute_force_corner_table(tmp_path):
    exe = str(tmp_path / "manifold_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "manifold_host_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(17)
    faces, base = [], 0
    for v, f in (to.fan(200, flip=(3, 77, 199)), to.fan(2, flip=(0,)), to.mobius(), mo.cones(5), ro.bowtie(), to.shared_edge_tetrahedra(), mo.disc(7, closed=True)):
        f = ro.flip_faces(f, np.nonzero(rng.random(len(f)) < 0.3)[0])
        f = np.array([np.roll(t, rng.integers(3)) for t in f])                   # every corner position at either end of an edge
        faces += (f + base).tolist()
        base += len(v) + 1000
    faces = np.array(faces, dtype=np.int64)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("=q", len(faces)) + faces.tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    n = 3 * len(faces)
    raw = open(dst, "rb").read()
    links, nm = np.frombuffer(raw, dtype=np.int64, count=n), np.frombuffer(raw, dtype=np.int32, count=n, offset=8 * n)
    assert len(raw) == 12 * n                                                    # the program compared them with its brute-force table and exited 0
    pairs, many = mo.corner_links(faces)
    got = sorted(((int(k) >> 32), (int(k) & 0xffffffff) >> 1) for k in links if k != me.INT64_MAX)
    assert got == sorted((min(a, b), max(a, b)) for a, b in pairs) and int(nm.sum()) == many == 2 and len(got) > 100
