"""CPU: the oracle of the mesh repair (tests/repair_oracle.py) on answers known by hand; the host logic of ``morig_amd.meshprep.repair`` /
``prepare_mesh(repair=True)`` on an emulated op layer (tests/repair_emulate.py through ``runtime._test_ops``) against that oracle; the new
exports' typing and refusals through the C ABI; and csrc/orient_core.h as the stand-alone program tools/meshfix_host_check.cpp, built
with the address and undefined-behaviour sanitizers and run as a program (never loaded into Python)."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import repair_emulate as re_
import repair_oracle as ro
import topology_oracle as to
from morig_amd import abi, meshprep, native, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops():
    emu = re_.RepairOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def outward(v, f):
    """every face's normal points away from the cube's centre"""
    c = v[f].mean(1) - 0.5
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return bool(((n * c).sum(1) > 0).all())


def open_strip(n_faces, flip=()):
    v, f = to.strip(n_faces + 2)
    return v, ro.flip_faces(f, flip)


# ------------------------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("subset", [(0,), (1, 4, 7, 10), (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11)])
def test_a_cube_with_flipped_faces_comes_back_outward(subset):
    v, f = ro.cube()
    assert outward(v, f)
    r = ro.repair(v, ro.flip_faces(f, subset))
    assert np.array_equal(r["faces"], f) and outward(v, r["faces"]) and sorted(np.nonzero(r["flipped"])[0]) == sorted(subset)
    o = ro.orientation(v, ro.flip_faces(f, subset))
    assert o["volume"][0] != 0 and (o["volume"][0] > 0) == (0 not in subset)     # S is taken relative to face 0; repaired, it is positive
    assert ro.orientation(v, r["faces"])["volume"][0] > 0
    rep = r["report"]
    assert rep["input"]["orientation_conflicts"] > 0 and to.diagnose(v, r["faces"])["orientation_conflicts"] == 0
    assert (rep["orientation_components"], rep["closed_components"], rep["flipped_faces"], rep["inverted_components"]) == (1, 1, len(subset), 0)


def test_an_inside_out_cube_is_one_inverted_component():
    v, f = ro.cube()
    r = ro.repair(v, ro.flip_faces(f, range(12)))
    assert r["report"]["inverted_components"] == 1 and r["flipped"].all() and np.array_equal(r["faces"], f)
    assert r["report"]["input"]["watertight"]                                    # it passed every check of the diagnosis


def test_a_moebius_strip_is_counted_and_left_alone():
    v, f = to.mobius()
    r = ro.repair(v, f, fill_holes="all")
    assert r["report"]["nonorientable_components"] == 1 and r["report"]["orientation_components"] == 1 and not r["flipped"].any()
    assert np.array_equal(r["faces"][:len(f)], f) and r["report"]["closed_components"] == 0


def test_orientation_does_not_cross_a_nonmanifold_edge():
    v, f = to.shared_edge_tetrahedra()
    r = ro.repair(v, ro.flip_faces(f, [4, 5, 6, 7]))                             # the second tetrahedron inside out
    rep = r["report"]
    assert rep["orientation_components"] == 2 and rep["closed_components"] == 0 and rep["boundary_loops"] == 0
    # both are open (the shared edge has four faces) and consistent in themselves: the majority rule flips nothing
    assert not r["flipped"].any() and rep["inverted_components"] == 0


def test_an_open_strip_follows_its_majority_and_keeps_the_root_on_a_tie():
    v, f = open_strip(9, flip=(2, 6))
    r = ro.repair(v, f)
    assert sorted(np.nonzero(r["flipped"])[0]) == [2, 6] and np.array_equal(r["faces"], to.strip(11)[1])
    v, f = open_strip(9, flip=(0, 1, 2, 3, 4, 5))                                 # the root face is in the minority now
    r = ro.repair(v, f)
    assert sorted(np.nonzero(r["flipped"])[0]) == [6, 7, 8]
    v, f = open_strip(8, flip=(0, 2, 4, 6))                                       # four against four: the root's side stays
    r = ro.repair(v, f)
    assert sorted(np.nonzero(r["flipped"])[0]) == [1, 3, 5, 7] and np.array_equal(r["faces"][0], f[0])
    v, f = open_strip(8, flip=(1, 3, 5, 7))
    assert sorted(np.nonzero(ro.repair(v, f)["flipped"])[0]) == [1, 3, 5, 7]


def test_a_cube_without_one_side_is_filled_watertight():
    v, f = ro.cube()
    r = ro.repair(v, f[2:], fill_holes="all")
    assert list(map(len, r["loops"].values())) == [4] and r["report"]["boundary_loops"] == 1 and r["report"]["filled_loops"] == 1
    assert (r["report"]["added_verts"], r["report"]["added_faces"]) == (1, 4) and np.array_equal(r["verts"][8], [0.0, 0.5, 0.5])
    before, after = to.diagnose(v, f[2:]), to.diagnose(r["verts"], r["faces"])
    assert after["watertight"] and after["euler"] == 2 == before["euler"] + 1 and outward(r["verts"], r["faces"])
    assert ro.repair(v, f[2:])["report"]["filled_loops"] == 0 and len(ro.repair(v, f[2:])["faces"]) == 10


def test_two_holes_that_touch_are_tangled_and_stay_open():
    v, f = ro.cube_two_holes_touching()
    r = ro.repair(v, f, fill_holes="all")
    assert r["report"]["tangled_boundary_edges"] == 6 and r["report"]["boundary_loops"] == 0 and r["report"]["added_faces"] == 0
    assert np.array_equal(r["faces"], f)
    v, f = ro.bowtie()
    r = ro.repair(v, f, fill_holes="all")
    assert r["report"]["tangled_boundary_edges"] == r["report"]["input"]["boundary_edges"] == 16 and r["report"]["filled_loops"] == 0


def test_fill_holes_by_length():
    v, f = ro.cube()
    f = ro.drop_faces(f, [0, 2, 3])                                              # a triangle hole and, on the opposite side, a square one
    lengths = sorted(len(l) for l in ro.repair(v, f)["loops"].values())
    assert lengths == [3, 4]
    r3, r4, rall = (ro.repair(v, f, fill_holes=x) for x in (3, 4, "all"))
    assert (r3["report"]["filled_loops"], r3["report"]["added_faces"], r3["report"]["boundary_loops"]) == (1, 3, 2)
    assert r4["report"]["filled_loops"] == 2 and np.array_equal(r4["faces"], rall["faces"]) and to.diagnose(rall["verts"], rall["faces"])["watertight"]
    assert to.diagnose(r3["verts"], r3["faces"])["boundary_edges"] == 4


def test_a_doubled_flat_sheet_has_no_volume_and_falls_to_the_majority():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 0]])
    top = [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)]
    v = np.concatenate([v, [[0.25, 0.5, 0.0]]])                                  # the lower sheet has a centre of its own, in the same plane
    f = np.array(top + [(1, 0, 5), (2, 1, 5), (3, 2, 5), (0, 3, 5)])
    o = ro.orientation(v, f)
    assert o["volume"][0] == 0.0 and not o["open_faces"] and o["count"]["closed_components"] == 1 and not o["flip"].any()
    r = ro.repair(v, ro.flip_faces(f, [1, 6]))
    assert sorted(np.nonzero(r["flipped"])[0]) == [1, 6] and r["report"]["inverted_components"] == 0 and r["report"]["closed_components"] == 1


# ------------------------------------------------------------------------------------------------------------------------- host logic
def cases():
    cv, cf = ro.cube()
    tv, tf = to.torus(6, 5)
    rng = np.random.default_rng(2)
    big_v, big_f = to.torus(9, 8)
    out = [("cube_flipped", (cv, ro.flip_faces(cf, (1, 4, 7, 10)))), ("cube_inverted", (cv, ro.flip_faces(cf, range(12)))),
           ("cube_holed", (cv, ro.flip_faces(ro.drop_faces(cf, [0, 2, 3]), (2, 3)))), ("moebius", to.mobius()),
           ("tetrahedra", (lambda m: (m[0], ro.flip_faces(m[1], (1, 5, 6))))(to.shared_edge_tetrahedra())),
           ("strip_tie", open_strip(8, (0, 2, 4, 6))), ("strip_random", (lambda m: (m[0], ro.flip_faces(m[1], (3, 9, 20))))(to.strip(40, "random", 4))),
           ("bowtie", ro.bowtie()), ("touching", ro.cube_two_holes_touching()), ("fan", to.fan(7, flip=(2, 5))),
           ("torus_disc_5", ro.torus_disc(6, 5, 5)),
           ("torus_two_discs", (big_v, ro.flip_faces(ro.drop_faces(big_f, [0, 1, 16, 70, 71, 86, 87]), rng.choice(130, 20, replace=False)))),
           ("torus_flipped", (tv, ro.flip_faces(tf, rng.choice(len(tf), 25, replace=False)))),
           ("raw", (np.concatenate([cv, cv[:2], [[9.0, 9, 9]]]), np.concatenate([ro.flip_faces(cf[2:], (3,)), [[8, 9, 3], [0, 0, 1], cf[5][[1, 2, 0]]]])))]
    return out


def same_result(got, want, report=None):
    v, f, vm, fm, fl = got
    assert v.dtype == torch.float64 and f.dtype == vm.dtype == fm.dtype == torch.int64 and fl.dtype == torch.bool
    assert np.array_equal(v.cpu().numpy(), want["verts"], equal_nan=True) and v.cpu().numpy().tobytes() == want["verts"].tobytes()
    for x, k in ((f, "faces"), (vm, "vertex_map"), (fm, "face_map"), (fl, "flipped")):
        assert np.array_equal(x.cpu().numpy(), want[k]), k
    if report is not None:
        for k in ro.FIELDS + ("orient_rounds",):
            assert report[k] == want["report"][k] and type(report[k]) is int, (k, report[k], want["report"][k])
        for k in to.FIELDS:
            assert report["input"][k] == want["report"]["input"][k], k


@pytest.mark.parametrize("orient,fill", [(True, None), (True, "all"), (True, 4), (False, "all"), (False, 3)])
def test_repair_on_the_emulated_ops_equals_the_oracle(ops, orient, fill):
    meshes = [m for _, m in cases()]
    out, reports = meshprep.repair([m[0] for m in meshes], [m[1] for m in meshes], orient=orient, fill_holes=fill, return_report=True)
    for (name, (v, f)), o, r in zip(cases(), out, reports):
        print(name, {k: r[k] for k in ro.FIELDS + ("orient_rounds",)})
        same_result(o, ro.repair(v, f, orient=orient, fill_holes=fill), r)
    assert tuple(reports[0])[:len(ro.FIELDS)] == meshprep.REPAIR_FIELDS == ro.FIELDS
    assert ("meshfix_orient_apply" in ops.calls) == orient and ("meshfix_fill_emit" in ops.calls) == (fill is not None)
    alone = meshprep.repair([meshes[2][0]], [meshes[2][1]], orient=orient, fill_holes=fill)          # a mesh alone: what it gives in the batch
    for x, y in zip(alone[0], out[2]):
        assert torch.equal(x, y)
    widest, third = max(len(to.clean(*m)[0]) for m in meshes), len(to.clean(*meshes[2])[0])
    assert ops.calls.count("meshfix_loop_round") == (widest - 1).bit_length() + 1 + (third - 1).bit_length() + 1   # ceil(log2(max nv)) + 1 per call


def test_keep_and_weld_go_to_clean(ops):
    cv, cf = ro.cube()
    v, f = np.concatenate([cv, cv + 3.0]), np.concatenate([ro.flip_faces(cf, (5,)), cf[2:] + 8])
    for keep in ("largest", 11, "all"):
        (o,), (r,) = meshprep.repair([v], [f], keep=keep, fill_holes="all", return_report=True)
        same_result(o, ro.repair(v, f, keep=keep, fill_holes="all"), r)
    sv, sf = to.split_cube()
    (o,), (r,) = meshprep.repair([sv], [ro.flip_faces(sf, (0, 1))], weld=False, return_report=True)
    same_result(o, ro.repair(sv, ro.flip_faces(sf, (0, 1)), weld=False), r)
    assert r["orientation_components"] == 6 and r["flipped_faces"] == 0 and r["boundary_loops"] == 6


def test_repair_is_idempotent(ops):
    for name, (v, f) in cases():
        for fill in (None, "all"):
            (a,) = meshprep.repair([v], [f], fill_holes=fill)
            (b,), (r,) = meshprep.repair([a[0]], [a[1]], fill_holes=fill, return_report=True)
            assert torch.equal(b[0], a[0]) and torch.equal(b[1], a[1]) and not b[4].any(), (name, fill)
            assert torch.equal(b[2], torch.arange(len(a[0]))) and torch.equal(b[3], torch.arange(len(a[1])))
            assert r["flipped_faces"] == r["added_faces"] == r["added_verts"] == 0


def test_list_shapes_of_empty_inputs(ops):
    assert meshprep.repair([], []) == [] and meshprep.repair([], [], return_report=True, fill_holes="all") == ([], [])
    assert not ops.calls
    e3, f3 = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    v, f = ro.cube()
    out, reps = meshprep.repair([e3, v, v], [f3, f[2:], f3], fill_holes="all", return_report=True)
    assert [tuple(o[0].shape) for o in out] == [(0, 3), (9, 3), (0, 3)] and [tuple(o[1].shape) for o in out] == [(0, 3), (14, 3), (0, 3)]
    assert [tuple(o[4].shape) for o in out] == [(0,), (14,), (0,)] and out[2][2].tolist() == [-1] * 8
    assert [r["orientation_components"] for r in reps] == [0, 1, 0] and [r["orient_rounds"] for r in reps] == [1, ro.repair(v, f[2:])["report"]["orient_rounds"], 1]
    (only,) = meshprep.repair([e3], [f3], fill_holes=3)
    assert tuple(only[0].shape) == (0, 3) and tuple(only[4].shape) == (0,)


def test_error_texts(ops):
    v, f = ro.cube()
    for bad in ("some", 2, -1, 2.5, True, "ALL"):
        with pytest.raises(ValueError, match="repair: fill_holes"):
            meshprep.repair([v], [f], fill_holes=bad)
    with pytest.raises(ValueError, match="clean: keep"):
        meshprep.repair([v], [f], keep="biggest")
    with pytest.raises(ValueError, match="clean: a face names a vertex outside its mesh"):
        meshprep.repair([v], [np.array([[0, 1, 8]])])
    assert not ops.calls                                                         # refused before any launch


def test_prepare_mesh_composes_the_maps_and_runs_later_stages_on_the_repaired_mesh(ops, monkeypatch):
    from morig_amd import geodesic, graph_build
    seen = {}
    monkeypatch.setattr(meshprep, "normalize", lambda verts: [(torch.as_tensor(v), np.zeros(3), 1.0) for v in verts])

    def simplify(verts, faces, target_faces):
        seen["simplify"] = [tuple(v.shape) for v in verts]
        return [(v[::2], f[:1] * 0, torch.arange(len(v)) // 2, 4) for v, f in zip(verts, faces)]
    monkeypatch.setattr(meshprep, "simplify", simplify)
    monkeypatch.setattr(meshprep, "tpl_edges", lambda faces, n, self_loops: seen.setdefault("tpl", list(n)) and [None] * len(n))
    monkeypatch.setattr(meshprep, "sample_surface", lambda v, f, **kw: seen.setdefault("sampled", [torch.as_tensor(x) for x in f]) and ([None] * len(v), [None] * len(v)))
    monkeypatch.setattr(meshprep, "voxelize", lambda v, f, dims: [None] * len(v))
    monkeypatch.setattr(geodesic, "surface_geodesic_batched", lambda v, p, n: [None] * len(v))
    monkeypatch.setattr(graph_build, "get_geo_edges_from_distance", lambda *a: None)
    v, f = cases()[-1][1]
    want = ro.repair(v, f, fill_holes="all")
    d = meshprep.prepare_mesh(v, f, repair=True)
    assert np.array_equal(d["vertex_map"].numpy(), want["vertex_map"]) and np.array_equal(d["faces"].numpy(), want["faces"])
    assert np.array_equal(d["flipped"].numpy(), want["flipped"]) and seen["tpl"] == [len(want["verts"])] and np.array_equal(seen["sampled"][0].numpy(), want["faces"])
    assert d["report"]["filled_loops"] == 1 and d["report"]["input"]["duplicate_verts"] == 2 and "simplify" not in seen
    assert "meshfix_fill_emit" in ops.calls and ops.calls.count("meshcheck_compact") == 1           # the clean step ran once, inside repair
    d = meshprep.prepare_mesh(v, f, repair=True, simplify_to=5)
    assert seen["simplify"] == [want["verts"].shape]
    assert np.array_equal(d["vertex_map"].numpy(), np.where(want["vertex_map"] >= 0, want["vertex_map"] // 2, -1))
    assert np.array_equal(d["flipped"].numpy(), want["flipped"])
    ops.calls.clear()
    d = meshprep.prepare_mesh(v, f)                                              # the default launches nothing new
    assert not ops.calls and "report" not in d and "flipped" not in d
    d = meshprep.prepare_mesh(v, f, clean=True)
    assert not any(c.startswith("meshfix_") for c in ops.calls) and "flipped" not in d


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_exports_are_typed_and_refuse_bad_arguments_without_a_device():
    names = [n for n in abi.SIGNATURES if n.startswith("morig_meshfix_")]
    assert len(names) == 10 and set(names) <= set(native.EXPORTS) and len(abi.STRUCTS) == 8       # plain parameters: no new argument struct
    assert abi.CONSTANTS["MORIG_ABI_VERSION"] == 3 and len([n for n in abi.SIGNATURES if n.startswith("morig_meshcheck_")]) == 12
    lib = native.load_library()
    K = abi.CONSTANTS
    for n in names:
        assert getattr(lib, n).argtypes is not None and hasattr(native.NativeOps, n[len("morig_"):])
    N = None
    calls = {                                                                     # name -> (arguments with a count of 4 everywhere, the count positions)
        "edge_records": ([N, 4, N, N, 1, 4, N, N, N, N, N], (1, 4, 5)),
        "links": ([N, N, 4, 4, N, N, N, N], (2, 3)),
        "orient_stats": ([N, N, 4, N, N, N, N, N], (2,)),
        "signed_volume": ([N, 4, N, N, 4, N, N, N, 4, N, N, N, N], (1, 4, 8)),
        "orient_apply": ([N, 4, N, N, 1, N, N, N, N, N, N, N, N, N, N, N], (1, 4)),
        "boundary_init": ([N, N, N, 4, N, 4, 4, N, N, N, N, N, N, N, N], (3, 5, 6)),
        "loop_round": ([N, N, 4, N, N, N], (2,)),
        "loop_centroid": ([N, 4, N, N, 4, N, 4, N, N], (1, 4, 6)),
        "fill_mark": ([N, N, N, 4, N, N], (3,)),
        "fill_emit": ([N, N, N, N, N, N, N, 4, 1, 4, N, N], (7, 8, 9)),
    }
    assert set(calls) == {n[len("morig_meshfix_"):] for n in names}
    for name, (args, counts) in calls.items():
        fn = getattr(lib, "morig_meshfix_" + name)
        assert len(args) == len(abi.SIGNATURES["morig_meshfix_" + name][1]), name
        assert fn(*args) == K["MORIG_E_INVALID"], name                            # null pointers
        for at in counts:
            bad = list(args)
            bad[at] = -1
            assert fn(*bad) == K["MORIG_E_INVALID"], (name, at)                   # a negative count
        zero = list(args)
        for at in counts:
            zero[at] = 0
        assert fn(*zero) == K["MORIG_OK"], name                                   # nothing to do: before anything is launched
    assert lib.morig_meshfix_fill_emit(N, N, N, N, N, N, N, 4, 1, 5, N, N) == K["MORIG_E_INVALID"]            # more faces than rows
    assert lib.morig_meshfix_loop_centroid(N, 4, N, N, 4, N, 5, N, N) == K["MORIG_E_INVALID"]                 # more chosen loops than loops
    assert lib.morig_meshfix_edge_records(N, (2 ** 31 - 257) // 8 + 1, N, N, 1, 4, N, N, N, N, N) == K["MORIG_E_INVALID"]   # 2 F + 6 F past the row limit
    assert K["MORIG_PROF_KINDS"] >= 96
    prof = [lib.morig_prof_name(k) for k in range(K["MORIG_PROF_KINDS"])]
    assert {b"meshfix_orient", b"meshfix_loops", b"meshfix_fill"} <= set(prof) and prof.index(b"meshfix_orient") == prof.index(b"meshcheck_compact") + 1


# ------------------------------------------------------------------------------------------------------------------------- the host program
def test_orient_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "meshfix_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "meshfix_host_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(13)
    # records: a 200-face fan edge with links on its neighbours, a conflict pair, a Moebius strip, a holed cube; sorted stably by key
    faces, base = [], 0
    for v, f in (to.fan(200, flip=(3, 77, 199)), to.fan(2, flip=(0, 1)), to.mobius(), (ro.cube()[0], ro.cube()[1][2:]), to.shared_edge_tetrahedra()):
        faces += (np.asarray(f) + base).tolist()
        base += len(v) + 1000
    faces = np.array(faces, dtype=np.int64)
    table = ro.edge_table(faces)
    keys = np.array(sorted((lo << 32) | hi for (lo, hi), r in table.items() for _ in r), dtype=np.int64)
    vals = np.array([(i << 1) | d for (lo, hi) in sorted(table) for i, d in table[(lo, hi)]], dtype=np.int32)
    keys, vals = np.concatenate([keys, [re_.INT64_MAX] * 2]), np.concatenate([vals, [-1, -1]]).astype(np.int32)
    tv, tf = to.torus(6, 5)
    tris = np.concatenate([tv[tf].reshape(-1, 9), rng.standard_normal((40, 9)) * 10.0 ** rng.integers(-150, 150, (40, 1)),
                           [[np.nan] * 9, [0.0] * 9, [-0.0, 1, 2, 3, -0.0, 5, 6, 7, -0.0], [1e200, 0, 0, 0, 1e200, 0, 0, 0, 1e200], [np.inf, 1, 1, 1, 2, 1, 1, 1, 3]]])
    decisions = [(tw, op, s, n, n1) for tw in (0, 1) for op in (0, 1) for s in (1.5, -1.5, 0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324)
                 for n, n1 in ((1, 0), (2, 1), (8, 0), (8, 3), (8, 4), (8, 5), (9, 4))]
    sums = [rng.standard_normal(n) * 10.0 ** rng.integers(-5, 5, n) for n in (0, 1, 12, 63, 64, 65, 129, 1000)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("=q", len(faces)) + faces.tobytes())
        fh.write(struct.pack("=q", len(keys)) + keys.tobytes() + vals.tobytes())
        fh.write(struct.pack("=q", len(tris)) + tris.astype(np.float64).tobytes())
        fh.write(struct.pack("=q", len(decisions)))
        for tw, op, s, n, n1 in decisions:
            fh.write(struct.pack("=qqdqq", tw, op, s, n, n1))
        fh.write(struct.pack("=q", len(sums)))
        for s in sums:
            fh.write(struct.pack("=q", len(s)) + s.astype(np.float64).tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    raw, at = open(dst, "rb").read(), 0

    def take(dtype, n):
        nonlocal at
        out = np.frombuffer(raw, dtype=dtype, count=n, offset=at)
        at += out.nbytes
        return out
    count, pos, cover = take(np.int32, len(keys)), take(np.int32, len(keys)), take(np.int64, len(keys))
    rkey, rval = take(np.int64, 3 * len(faces)), take(np.int32, 3 * len(faces))
    t, tneg = take(np.float64, len(tris)), take(np.float64, len(tris))
    cls, byvol, info = take(np.int32, len(decisions)), take(np.int32, len(decisions)), take(np.int32, len(decisions))
    folded = take(np.float64, len(sums))
    assert at == len(raw)
    # the records of every face, then the shape of every run and the cover edges of the links, by the dict of edges
    want = [((min(a, b) << 32) | max(a, b), (i << 1) | int(a < b)) for i, f in enumerate(faces.tolist()) for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0]))]
    assert rkey.tolist() == [w[0] for w in want] and rval.tolist() == [w[1] for w in want]
    i, seen = 0, set()
    for (lo, hi) in sorted(table):
        run = table[(lo, hi)]
        for p, _ in enumerate(run):
            assert count[i + p] == min(len(run), 3) and pos[i + p] == min(p, 2), (lo, hi, p)
            if len(run) == 2:
                (f, df), (g, dg) = run
                assert cover[i + p] == ((2 * f + p) << 32) | ((2 * g + (p ^ int(df == dg))) << 1)
            else:
                assert cover[i + p] == re_.INT64_MAX
        seen.add(min(len(run), 3))
        i += len(run)
    assert seen == {1, 2, 3} and 200 in [len(r) for r in table.values()] and (cover[-2:] == re_.INT64_MAX).all()
    # t(f) bit for bit, and its exact negation under the exchange of corners 1 and 2
    with np.errstate(all="ignore"):
        want_t = np.array([ro.term(x.reshape(3, 3), (0, 1, 2)) for x in tris])
    assert np.array_equal(t, want_t, equal_nan=True) and np.array_equal(tneg, -want_t, equal_nan=True) and np.isnan(t).sum() >= 1
    live = ~np.isnan(t) & (t != 0)
    assert np.array_equal(np.signbit(tneg[live]), ~np.signbit(t[live])) and live.sum() > 60
    # the decision, by the sentences of the rule
    for k, (tw, op, s, n, n1) in enumerate(decisions):
        if tw:
            assert (cls[k], byvol[k], info[k]) == (-1, 0, 2)
            continue
        vol = not op and (s > 0 or s < 0)
        c = (1 if s > 0 else 0) if vol else (1 if n1 <= n - n1 else 0)
        turned = n1 if c == 1 else n - n1
        assert (cls[k], byvol[k], info[k]) == (c, int(vol), 1 | (0 if op else 4) | (8 if vol and turned == n else 0)), (tw, op, s, n, n1)
    assert folded.tolist() == [to.lane_sum(s.tolist()) for s in sums]
