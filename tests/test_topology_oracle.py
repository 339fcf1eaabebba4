"""CPU: the oracle of the mesh diagnosis (tests/topology_oracle.py) on answers known by hand; the restated component round against
union-find, with its round counts; the stated order of the area sum against ``math.fsum``; the host logic of
``morig_amd.meshprep.diagnose`` / ``clean`` / ``prepare_mesh(clean=True)`` on an emulated op layer (tests/topology_emulate.py through
``runtime._test_ops``); the new exports' typing and refusals through the C ABI; and csrc/topo_core.h as the stand-alone program
tools/topo_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program (never loaded into Python)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import topology_emulate as te
import topology_oracle as to
from morig_amd import abi, meshprep, native, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ascending", "descending", "zigzag", "random")


@pytest.fixture()
def ops():
    emu = te.TopologyOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def generators():
    out = [("cube", to.cube()), ("split_cube", to.split_cube()), ("torus", to.torus(8, 6)), ("mobius", to.mobius()),
           ("tetrahedra", to.shared_edge_tetrahedra()), ("fan", to.fan(7, flip=(2, 5)))]
    out += [(f"strip_{n}_{k}", to.strip(n, k, seed=n)) for n in (65, 1025) for k in KINDS]
    out.append(("torus_random", to.torus(16, 16, perm=np.random.default_rng(3).permutation(256))))
    return out


# ------------------------------------------------------------------------------------------------------------------------- known answers
def test_known_answers():
    c = to.diagnose(*to.cube())
    assert c["euler"] == 2 and c["watertight"] and (c["verts"], c["edges"], c["faces"], c["components"]) == (8, 18, 12, 1)
    t = to.diagnose(*to.torus(8, 6))
    assert t["euler"] == 0 and t["watertight"] and t["components"] == 1
    s = to.diagnose(*to.split_cube(), weld=False)
    assert s["boundary_edges"] == 24 and not s["watertight"] and s["components"] == 6 and s["duplicate_verts"] == 0
    s = to.diagnose(*to.split_cube())
    assert s["watertight"] and s["euler"] == 2 and s["duplicate_verts"] == 16 and s["components"] == 1
    m = to.diagnose(*to.mobius())
    assert m["orientation_conflicts"] >= 1 and m["nonmanifold_edges"] == 0 and not m["watertight"]
    d = to.diagnose(*to.shared_edge_tetrahedra())
    assert d["nonmanifold_edges"] == 1 and d["edge_table"][(0, 1)][0] == 4 and d["boundary_edges"] == 0 and not d["watertight"]


def test_weld_is_exact_and_spares_what_is_not_finite():
    v = np.array([[0.0, 0, 0], [-0.0, 0.0, -0.0], [np.nan, 0, 0], [np.nan, 0, 0], [np.inf, 1, 1], [np.inf, 1, 1], [1e-300, 0, 0], [1, 1, 1], [1, 1, 1]])
    assert to.weld_rep(v).tolist() == [0, 0, 2, 3, 4, 5, 6, 7, 7] and to.weld_rep(v, weld=False).tolist() == list(range(9))
    d = to.diagnose(v, [[0, 1, 7], [0, 6, 7], [6, 0, 8], [2, 3, 4]])
    assert (d["nonfinite_verts"], d["duplicate_verts"], d["degenerate_faces"], d["duplicate_faces"], d["faces"]) == (4, 2, 1, 1, 2)
    assert d["surv"].tolist() == [-1, 1, 1, 3]


# ------------------------------------------------------------------------------------------------------------------------- the round
@pytest.mark.parametrize("name,mesh", generators(), ids=[g[0] for g in generators()])
def test_the_restated_round_gives_the_union_find_labels_within_its_round_bound(name, mesh):
    d = to.diagnose(*mesh)
    assert np.array_equal(d["labels"], d["labels_by_rounds"])
    bound = math.ceil(math.log2(len(mesh[0]))) + 8
    print(f"{name}: {len(mesh[0])} vertices, {d['rounds']} rounds (bound {bound})")
    assert d["rounds"] <= bound


def test_round_counts_of_long_paths_stay_logarithmic():
    for n in (4096,):
        for k in KINDS:
            pairs = {(min(a, b), max(a, b)) for a, b in zip(to.numbering(n, k, 1)[:-1], to.numbering(n, k, 1)[1:])}
            lab, rounds = to.cc_rounds(n, pairs)
            print(f"path {n} {k}: {rounds} rounds")
            assert not lab.any() and rounds <= math.ceil(math.log2(n)) + 8


# ------------------------------------------------------------------------------------------------------------------------- the area order
def test_the_stated_sum_order_is_within_its_bound_of_fsum():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 200, 4097):
        a = (rng.random(n) * 10.0 ** rng.integers(-8, 8, n)).tolist()
        got, want = to.lane_sum(a), math.fsum(a)
        bound = (n - 1) * 2.0 ** -53 * math.fsum(abs(x) for x in a)
        print(f"n = {n}: |lane_sum - fsum| = {abs(got - want):.3e}, bound {bound:.3e}")
        assert abs(got - want) <= bound


# ------------------------------------------------------------------------------------------------------------------------- host logic
def same_report(got, want):
    for k in to.FIELDS + ("watertight", "rounds"):
        assert got[k] == want[k] and type(got[k]) is (bool if k == "watertight" else int), (k, got[k], want[k])
    assert tuple(got)[:len(to.FIELDS)] == meshprep.REPORT_FIELDS == to.FIELDS


def test_diagnose_on_the_emulated_ops_equals_the_oracle(ops):
    meshes = [m for _, m in generators()[:8]]
    for weld in (True, False):
        reps = meshprep.diagnose([m[0] for m in meshes], [m[1] for m in meshes], weld=weld, return_components=True)
        for (v, f), r in zip(meshes, reps):
            w = to.diagnose(v, f, weld)
            same_report(r, w)
            for k in ("root", "verts", "faces", "boundary_edges", "area"):
                assert np.array_equal(r["component_table"][k].numpy(), w["component_table"][k]), k
            assert np.array_equal(r["boundary_edge_list"].numpy(), w["boundary_edge_list"])
    assert "component_table" not in meshprep.diagnose([meshes[0][0]], [meshes[0][1]])[0]
    assert ops.calls.count("meshcheck_edge_classify") == 3


def two_part_mesh():
    """a cube, a split cube beside it, a lone triangle, an isolated vertex, a degenerate face and a duplicate of face 0"""
    (cv, cf), (sv, sf) = to.cube(), to.split_cube()
    v = np.concatenate([cv, sv + 5.0, [[9.0, 9, 9], [9, 10, 9], [9, 9, 10], [20, 20, 20]]])
    f = np.concatenate([cf, sf + 8, [[32, 33, 34], [0, 0, 1], cf[0][[1, 2, 0]]]])
    return v, f


@pytest.mark.parametrize("keep", ["all", "largest", 0, 1, 2, 12, 13])
@pytest.mark.parametrize("drop", [True, False])
def test_clean_keep_rules_with_ties_and_idempotence(ops, keep, drop):
    meshes = [two_part_mesh(), to.torus(5, 4), to.mobius()]
    out, reports = meshprep.clean([m[0] for m in meshes], [m[1] for m in meshes], keep=keep, drop_unreferenced=drop, return_report=True)
    for (v, f), o, r in zip(meshes, out, reports):
        for x, y in zip(o, to.clean(v, f, True, keep, drop)):
            assert x.dtype == (torch.float64 if x.is_floating_point() else torch.int64) and np.array_equal(x.numpy(), y)
        same_report(r, to.diagnose(v, f))
        again, = meshprep.clean([o[0]], [o[1]], drop_unreferenced=drop)
        assert torch.equal(again[0], o[0]) and torch.equal(again[1], o[1])
        assert torch.equal(again[2], torch.arange(len(o[0]))) and torch.equal(again[3], torch.arange(len(o[1])))
    if keep == "largest":                                                        # two components of 12 faces: the lower label wins
        assert out[0][1].shape[0] == 12 and out[0][2][:8].tolist() == list(range(8)) and (out[0][2][8:] == -1).all() == drop
        assert out[0][3][-1] == out[0][3][0] == 0 and out[0][3][-2] == -1        # the duplicate points to its survivor, the degenerate nowhere


def test_list_shapes_of_empty_inputs(ops):
    assert meshprep.diagnose([], []) == [] and meshprep.clean([], []) == [] and meshprep.clean([], [], return_report=True) == ([], [])
    assert not ops.calls
    e3, f3 = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    v, f = to.cube()
    reps = meshprep.diagnose([e3, v, v], [f3, f, f3], return_components=True)
    assert [r["faces"] for r in reps] == [0, 12, 0] and [r["components"] for r in reps] == [0, 1, 0] and reps[2]["unreferenced_verts"] == 8
    assert not reps[0]["watertight"] and reps[0]["rounds"] == 1 and reps[0]["component_table"]["area"].shape == (0,)
    out = meshprep.clean([e3, v, v], [f3, f, f3])
    assert [tuple(o[0].shape) for o in out] == [(0, 3), (8, 3), (0, 3)] and [tuple(o[1].shape) for o in out] == [(0, 3), (12, 3), (0, 3)]
    assert out[2][2].tolist() == [-1] * 8 and tuple(out[0][2].shape) == (0,) and tuple(out[0][3].shape) == (0,)
    only = meshprep.clean([e3], [f3], keep="largest")
    assert tuple(only[0][0].shape) == (0, 3)


def test_error_texts(ops):
    v, f = to.cube()
    with pytest.raises(ValueError, match="diagnose: a face names a vertex outside its mesh"):
        meshprep.diagnose([v], [np.array([[0, 1, 8]])])
    with pytest.raises(ValueError, match="clean: a face names a vertex outside its mesh"):
        meshprep.clean([v], [np.array([[0, -1, 2]])])
    assert not ops.calls                                                         # refused before any launch
    for bad in ("biggest", -1, 2.5, True, None):
        with pytest.raises(ValueError, match="clean: keep"):
            meshprep.clean([v], [f], keep=bad)


def test_the_round_guard_ends_the_loop():
    runtime._test_ops = te.TopologyOps(stall_rounds=True)
    try:
        v, f = to.cube()
        with pytest.raises(RuntimeError, match=r"diagnose: the component loop passed its bound of 10 rounds \(status 2\)"):
            meshprep.diagnose([v], [f])
        assert runtime._test_ops.calls.count("meshcheck_cc_round") == 10
    finally:
        runtime._test_ops = None


def test_prepare_mesh_composes_the_maps_and_runs_later_stages_on_the_cleaned_mesh(ops, monkeypatch):
    from morig_amd import geodesic, graph_build
    seen = {}
    monkeypatch.setattr(meshprep, "normalize", lambda verts: [(torch.as_tensor(v), np.zeros(3), 1.0) for v in verts])

    def simplify(verts, faces, target_faces):
        seen["simplify"] = [tuple(v.shape) for v in verts]
        return [(v[::2], f[:1] * 0, torch.arange(len(v)) // 2, 4) for v, f in zip(verts, faces)]
    monkeypatch.setattr(meshprep, "simplify", simplify)
    monkeypatch.setattr(meshprep, "tpl_edges", lambda faces, n, self_loops: seen.setdefault("tpl", list(n)) and [None] * len(n))
    monkeypatch.setattr(meshprep, "sample_surface", lambda v, f, **kw: ([None] * len(v), [None] * len(v)))
    monkeypatch.setattr(meshprep, "voxelize", lambda v, f, dims: [None] * len(v))
    monkeypatch.setattr(geodesic, "surface_geodesic_batched", lambda v, p, n: [None] * len(v))
    monkeypatch.setattr(graph_build, "get_geo_edges_from_distance", lambda *a: None)
    v, f = two_part_mesh()
    d = meshprep.prepare_mesh(v, f, clean=True)
    want = to.clean(v, f)
    assert np.array_equal(d["vertex_map"].numpy(), want[2]) and np.array_equal(d["faces"].numpy(), want[1]) and seen["tpl"] == [len(want[0])]
    assert d["report"]["duplicate_verts"] == 16 and d["report"]["components"] == 3 and "simplify" not in seen
    d = meshprep.prepare_mesh(v, f, clean=True, simplify_to=5)
    assert seen["simplify"] == [want[0].shape]
    assert np.array_equal(d["vertex_map"].numpy(), np.where(want[2] >= 0, want[2] // 2, -1)) and d["verts"].shape[0] == (len(want[0]) + 1) // 2
    ops.calls.clear()
    d = meshprep.prepare_mesh(v, f)                                              # the default launches nothing new
    assert not ops.calls and "report" not in d and "vertex_map" not in d


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_exports_are_typed_and_refuse_bad_arguments_without_a_device():
    names = [n for n in abi.SIGNATURES if n.startswith("morig_meshcheck_")]
    assert len(names) == 12 and set(names) <= set(native.EXPORTS) and len(abi.STRUCTS) == 8      # plain parameters: no new argument struct
    assert abi.CONSTANTS["MORIG_ABI_VERSION"] == 3
    lib = native.load_library()
    K = abi.CONSTANTS
    for n in names:
        assert getattr(lib, n).argtypes is not None and hasattr(native.NativeOps, n[len("morig_"):])
    N = None
    calls = {                                                                     # name -> (arguments with a count of 4 everywhere, the count positions)
        "coord_keys": ([N, 4, N, N, N], (1,)),
        "weld_mark": ([N, N, N, 4, N, 1, N, N], (3, 5)),
        "run_rep": ([N, N, N, N, 4, N, N, N], (4,)),
        "face_keys": ([N, 4, N, N, 1, N, 4, N, N, N, N, N, N], (1, 4, 6)),
        "face_mark": ([N, N, N, 4, N, N], (3,)),
        "face_edges": ([N, 4, N, N, 4, N, N, N, N], (1, 4)),
        "cc_round": ([N, N, 4, N, 4, N, 1, N, N], (2, 4, 6)),
        "edge_classify": ([N, 4, N, 4, N, N, N], (1, 3)),
        "comp_counts": ([N, N, 4, N, N, 4, N, N, N, N], (2, 5)),
        "comp_area": ([N, 4, N, 4, N, N, 4, N, N], (1, 3, 6)),
        "keep_flags": ([N, N, N, N, 1, 4, N, N, 4, N, N, N], (5, 8)),
        "compact": ([N, N, N, N, N, N, 4, 1, N, N, N, N, N, N, 4, 2, 2, N, N, N, N, N], (6, 7, 14, 15, 16)),
    }
    assert set(calls) == {n[len("morig_meshcheck_"):] for n in names}
    for name, (args, counts) in calls.items():
        fn = getattr(lib, "morig_meshcheck_" + name)
        assert fn(*args) == K["MORIG_E_INVALID"], name                            # null pointers
        for at in counts:
            bad = list(args)
            bad[at] = -1
            assert fn(*bad) == K["MORIG_E_INVALID"], (name, at)                   # a negative count
        zero = list(args)
        for at in counts:
            zero[at] = 0
        assert fn(*zero) == K["MORIG_OK"], name                                   # nothing to do: before anything is launched
    assert lib.morig_meshcheck_compact(N, N, N, N, N, N, 4, 1, N, N, N, N, N, N, 4, 5, 2, N, N, N, N, N) == K["MORIG_E_INVALID"]   # more out than in
    prof = [lib.morig_prof_name(k) for k in range(K["MORIG_PROF_KINDS"])]
    assert {b"meshcheck_weld", b"meshcheck_faces", b"meshcheck_edges", b"meshcheck_components", b"meshcheck_compact"} <= set(prof)


# ------------------------------------------------------------------------------------------------------------------------- the host program
def test_topo_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "topo_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "topo_host_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(11)
    xs = np.concatenate([[0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1.0, -1.0, np.finfo(np.float64).max,
                          -np.finfo(np.float64).max], rng.standard_normal(200) * 10.0 ** rng.integers(-300, 300, 200)])
    # edge keys: a 200-face fan on one edge (with flipped faces), the shapes with a conflict and a non-manifold edge, and the sentinel
    keys = []
    for v, f in (to.fan(200, flip=(3, 77, 199)), to.mobius(), to.shared_edge_tetrahedra(), to.cube(), to.fan(2, flip=(0, 1)), to.fan(2)):
        base = len(keys) * 1000
        for t in f:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                a, b = int(a) + base, int(b) + base
                keys.append((a << 32) | (b << 1) | 1 if a < b else (b << 32) | (a << 1))
    keys = np.array(sorted(keys) + [te.INT64_MAX] * 3, dtype=np.int64)
    tv, tf = to.torus(6, 5)
    tris = np.concatenate([tv[tf].reshape(-1, 9), [[0, 0, 0, 1, 1, 1, 2, 2, 2], [1, 2, 3, 1, 2, 3, 4, 4, 4], [0, 0, 0, np.inf, 0, 0, 0, 1, 0],
                                                  [np.nan] * 9, [1e200, 0, 0, 0, 1e200, 0, 0, 0, 1e200], [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]]])
    sums = [rng.random(n) * 10.0 ** rng.integers(-5, 5, n) for n in (0, 1, 63, 64, 65, 200, 1000)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("=q", len(xs)) + xs.astype(np.float64).tobytes())
        fh.write(struct.pack("=q", len(keys)) + keys.tobytes())
        fh.write(struct.pack("=q", len(tris)) + tris.astype(np.float64).tobytes())
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
    ckeys, fin, cls, run_len = take(np.int64, len(xs)), take(np.int32, len(xs)), take(np.int32, len(keys)), take(np.int64, len(keys))
    area, zero, folded = take(np.float64, len(tris)), take(np.int32, len(tris)), take(np.float64, len(sums))
    assert at == len(raw)
    # the coordinate key: that of the emulation, equal exactly for equal numbers, ordered as the numbers
    assert ckeys.tolist() == [te.coord_key(float(x)) for x in xs] and np.array_equal(fin != 0, np.isfinite(xs))
    ok = np.isfinite(xs)
    a, b = np.meshgrid(np.nonzero(ok)[0], np.nonzero(ok)[0])
    assert np.array_equal(xs[a] < xs[b], ckeys[a] < ckeys[b]) and np.array_equal(xs[a] == xs[b], ckeys[a] == ckeys[b]) and ckeys[0] == ckeys[1] == 0
    # the classes of the runs: a dict per edge
    table = {}
    for k in keys[:-3].tolist():
        n, fw = table.get(k >> 1, (0, 0))
        table[k >> 1] = (n + 1, fw + (k & 1))
    want_cls, want_len = np.zeros(len(keys), dtype=np.int32), np.zeros(len(keys), dtype=np.int64)
    for i, k in enumerate(keys[:-3].tolist()):
        if i == 0 or keys[i - 1] >> 1 != k >> 1:
            n, fw = table[k >> 1]
            want_len[i], want_cls[i] = n, 2 if n == 1 else 3 if n >= 3 else 1 if fw == 1 else 4
    assert np.array_equal(cls, want_cls) and np.array_equal(run_len, want_len)
    assert 200 in run_len and set(cls.tolist()) == {0, 1, 2, 3, 4} and sorted(run_len[cls == 4].tolist()) == [2, 2, 2]
    # areas bit for bit (NaN where the oracle has NaN), and the fold
    want_area = np.array([to.face_area(t.reshape(3, 3), (0, 1, 2)) for t in tris])
    assert np.array_equal(area, want_area, equal_nan=True)
    assert zero.tolist() == [1 if all(x == 0.0 for x in to.normal(t.reshape(3, 3), 0, 1, 2)) else 0 for t in tris] and zero[-6] == 1 and zero[-5] == 1
    assert folded.tolist() == [to.lane_sum(s.tolist()) for s in sums]
