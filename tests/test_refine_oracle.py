"""CPU: the oracle of the mesh refinement (tests/refine_oracle.py) on its invariants; the host logic of ``morig_amd.meshprep.refine`` /
``interpolate`` / ``prepare_mesh(refine_...)`` on an emulated op layer (tests/refine_emulate.py through ``runtime._test_ops``) against that
oracle; the new exports' typing and refusals through the C ABI; and csrc/split_core.h as the stand-alone program
tools/refine_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program (never loaded into Python)."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import refine_emulate as fe
import refine_oracle as fo
import topology_oracle as to
from morig_amd import abi, meshprep, native, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops():
    emu = fe.RefineOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def meshes():
    return [("torus", to.torus(6, 5)), ("torus_thin", to.torus(9, 4)), ("box", fo.box(1.0, 0.13, 2.7)), ("cube", fo.box()), ("fan", to.fan(5)),
            ("disc", fo.disc(9)), ("disc_big", fo.disc(14)), ("seam", to.split_cube()), ("tetrahedra", to.shared_edge_tetrahedra())]


SETTINGS = (dict(max_edge=0.45), dict(min_verts=150), dict(max_edge=0.7, min_verts=120))


# ------------------------------------------------------------------------------------------------------------------------- invariants
def test_the_figures_of_the_rule_on_three_boxes():
    r = fo.refine(*fo.box(1.0, 0.13, 2.7), min_verts=1000)["report"]
    assert (r["passes"], r["verts"], r["converged"]) == (5, 1000, True)
    r = fo.refine(*fo.box(), max_edge=0.3)["report"]
    assert (r["passes"], r["verts"], r["faces"], r["converged"]) == (3, 194, 384, True)
    r = fo.refine(*fo.box(1.0, 0.13, 2.7), max_edge=0.06)["report"]
    assert (r["passes"], r["verts"], r["converged"]) == (6, 9602, True)


@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("name,mesh", meshes(), ids=[n for n, _ in meshes()])
def test_refinement_keeps_topology_area_and_volume(name, mesh, kw):
    v, f = mesh
    r = fo.refine(v, f, **kw)
    rep, V = r["report"], len(v)
    before, after = to.diagnose(v, f, weld=False), to.diagnose(r["verts"], r["faces"], weld=False)
    for k in ("euler", "components", "watertight", "orientation_conflicts", "unreferenced_verts", "degenerate_faces", "duplicate_faces"):
        assert after[k] == before[k], k
    split_boundary = split_fans = 0
    for faces, marked in r["history"]:                                          # every split edge by its class in the mesh it was split in
        n = fo.edge_classes(faces)
        split_boundary += sum(1 for e in marked if n[e] == 1)
        split_fans += sum(1 for e in marked if n[e] >= 3)
    assert after["boundary_edges"] == before["boundary_edges"] + split_boundary
    assert after["nonmanifold_edges"] == before["nonmanifold_edges"] + split_fans
    assert rep["verts"] == V + sum(rep["edges_split"]) and rep["faces"] == len(f) + rep["faces_split_1"] + 2 * rep["faces_split_2"] + 3 * rep["faces_split_3"]
    a0, a1, s0, s1 = fo.area(v, f), fo.area(r["verts"], r["faces"]), fo.signed_volume(v, f), fo.signed_volume(r["verts"], r["faces"])
    print(name, kw, rep["passes"], rep["verts"], "area ulps", abs(a1 - a0) / np.spacing(a0), "volume ulps", abs(s1 - s0) / np.spacing(max(abs(s0), 5e-324)))
    assert abs(a1 - a0) <= 64 * np.spacing(a0)
    assert abs(s1 - s0) <= 64 * np.spacing(abs(s0)) or (s0 == 0.0 and abs(s1) <= 64 * np.spacing(a0))   # an open flat sheet has no volume
    assert np.array_equal(r["verts"][:V], v) and np.array_equal(r["parents"][:V], np.stack([np.arange(V)] * 2, 1))
    assert (r["parents"][V:].max(1) < np.arange(V, rep["verts"])).all() and (np.diff(r["face_map"]) >= 0).all()
    assert np.array_equal(r["verts"][V:], 0.5 * (r["verts"][r["parents"][V:, 0]] + r["verts"][r["parents"][V:, 1]]))
    assert rep["converged"] and not rep["stalled"]
    if "max_edge" in kw and "min_verts" not in kw:
        assert fo.longest_edge2(r["verts"], r["faces"]) <= kw["max_edge"] ** 2
    if "min_verts" in kw:
        assert rep["verts"] == max(kw["min_verts"], rep["verts"]) and (rep["verts"] == kw["min_verts"] or "max_edge" in kw)
    if kw == dict(min_verts=150):
        assert rep["verts"] == 150


def test_the_longest_edge_shrinks_every_pass():
    for _, (v, f) in meshes():
        r = fo.refine(v, f, max_edge=0.2)
        tops = []
        for faces, marked in r["history"]:
            tops.append(fo.longest_edge2(r["verts"], faces))                      # the rows of a pass are a prefix of the final rows
        tops.append(fo.longest_edge2(r["verts"], r["faces"]))
        assert all(b < a for a, b in zip(tops, tops[1:])) and tops[-1] <= 0.2 * 0.2


def test_duplicated_seams_weld_to_the_mesh_that_refining_the_welded_mesh_gives():
    sv, sf = to.split_cube()
    wv, wf = to.clean(sv, sf)[:2]
    assert len(sv) == 24 and len(wv) == 8
    a, b = fo.refine(sv, sf, max_edge=0.3), fo.refine(wv, wf, max_edge=0.3)
    assert a["report"]["faces_split_2"] == b["report"]["faces_split_2"] == 0      # no diagonal is chosen, so no tie falls to a vertex number
    av, af = to.clean(a["verts"], a["faces"])[:2]
    shape = lambda v, f: sorted(tuple(sorted(map(tuple, v[t]))) for t in f)
    assert len(av) == b["report"]["verts"] == 194 and shape(av, af) == shape(b["verts"], b["faces"])
    assert to.diagnose(a["verts"], a["faces"])["watertight"] and not to.diagnose(a["verts"], a["faces"], weld=False)["watertight"]


def test_what_the_oracle_does_with_damaged_and_finished_meshes():
    v, f = fo.box()
    with pytest.raises(ValueError, match="refine: a face names a vertex outside its mesh"):
        fo.refine(v, np.array([[0, 1, 8]]), max_edge=1.0)
    with pytest.raises(ValueError, match="refine: give max_edge"):
        fo.refine(v, f)
    r = fo.refine(v, f, min_verts=8)
    assert r["report"]["passes"] == 0 and r["report"]["converged"] and np.array_equal(r["faces"], f)
    r = fo.refine(np.zeros((4, 3)), np.array([[0, 1, 2], [1, 2, 3]]), min_verts=9)["report"]
    assert r["stalled"] and not r["converged"] and r["verts"] == 4
    r = fo.refine(v, f, max_edge=0.3, max_passes=2)["report"]
    assert (r["passes"], r["converged"]) == (2, False)


# ------------------------------------------------------------------------------------------------------------------------- host logic
class Reads:
    """counts the calls that bring a device value to the host"""

    def __init__(self, monkeypatch):
        self.n = 0
        for name in ("cpu", "item", "tolist", "nonzero"):
            monkeypatch.setattr(torch.Tensor, name, self._counting(getattr(torch.Tensor, name)))
        monkeypatch.setattr(torch, "nonzero", self._counting(torch.nonzero))

    def _counting(self, fn):
        def wrapped(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        return wrapped


def same_result(got, want, report=None):
    v, f, p, m = got
    assert v.dtype == torch.float64 and f.dtype == p.dtype == m.dtype == torch.int64
    assert v.numpy().tobytes() == want["verts"].tobytes()
    for x, k in ((f, "faces"), (p, "parents"), (m, "face_map")):
        assert np.array_equal(x.numpy(), want[k]) and tuple(x.shape) == want[k].shape, k
    if report is not None:
        assert report == want["report"] and tuple(report) == meshprep.REFINE_FIELDS == fo.REPORT_KEYS


@pytest.mark.parametrize("kw", SETTINGS + (dict(max_edge=0.45, max_passes=2), dict(min_verts=90, max_passes=1)), ids=str)
def test_refine_on_the_emulated_ops_equals_the_oracle(ops, kw):
    ms = [m for _, m in meshes()] + [(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)), (np.full((3, 3), np.nan), np.array([[0, 1, 2]]))]
    out, reports = meshprep.refine([m[0] for m in ms], [m[1] for m in ms], return_report=True, **kw)
    for m, o, r in zip(ms, out, reports):
        same_result(o, fo.refine(*m, **kw), r)
    alone, report = meshprep.refine(ms[2][0], ms[2][1], return_report=True, **kw)   # a mesh alone: what it gives in the batch
    for x, y in zip(alone, out[2]):
        assert torch.equal(x, y)
    assert report == reports[2] and len(meshprep.refine(ms[2][0], ms[2][1], **kw)) == 4


def test_one_pass_is_one_list_of_calls_and_one_host_read(ops, monkeypatch):
    v, f = fo.box()
    batch = ([v, v * 0.5], [f, f])
    reads = Reads(monkeypatch)
    out, reports = meshprep.refine(*batch, max_edge=0.4, return_report=True)
    one_pass = ["refine_edge_records", "tpl_edge_flags", "refine_mark", "refine_number", "refine_pattern"]
    # the big cube splits twice, the small one once; the third look finds nothing and emits nothing
    assert [r["passes"] for r in reports] == [2, 1]
    assert ops.calls == (one_pass + ["refine_emit"]) * 2 + one_pass and reads.n == 3
    ops.calls.clear()
    reads.n = 0
    out, reports = meshprep.refine(*batch, max_edge=0.4, min_verts=120, return_report=True)
    looks = ops.calls.count("refine_edge_records")
    # a mesh whose look finds no long edge moves on to the count; only the looks with a mesh in the count have a budget
    assert reads.n == looks and 0 < ops.calls.count("refine_budget") < looks and ops.calls.count("refine_emit") <= looks
    assert [r["verts"] for r in reports] == [120, 120] and all(r["converged"] for r in reports)
    ops.calls.clear()
    out, reports = meshprep.refine(*batch, min_verts=8, return_report=True)       # nothing to do: nothing is launched
    assert not ops.calls and all(r["converged"] and r["passes"] == 0 for r in reports) and torch.equal(out[1][1], torch.from_numpy(f))


def test_list_shapes_and_error_texts(ops):
    assert meshprep.refine([], [], max_edge=1.0) == [] and meshprep.refine([], [], min_verts=5, return_report=True) == ([], [])
    v, f = fo.box()
    for kw, text in ((dict(), "refine: give max_edge, min_verts or both"), (dict(max_edge=0.0), "refine: max_edge"), (dict(max_edge=np.inf), "refine: max_edge"),
                     (dict(max_edge="long"), "refine: max_edge"), (dict(min_verts=-1), "refine: min_verts"), (dict(min_verts=2.5), "refine: min_verts"),
                     (dict(max_edge=1.0, max_passes=-1), "refine: max_passes"), (dict(min_verts=True), "refine: min_verts")):
        with pytest.raises(ValueError, match=text):
            meshprep.refine([v], [f], **kw)
    assert not ops.calls                                                         # refused before any launch
    with pytest.raises(ValueError, match="refine: a face names a vertex outside its mesh"):
        meshprep.refine([v, v], [f, np.array([[0, 1, 8]])], max_edge=0.5)
    with pytest.raises(ValueError, match="refine: a face names a vertex outside its mesh"):
        meshprep.refine(v, np.array([[0, -1, 2]]), min_verts=20)
    assert "refine_emit" not in ops.calls                                        # the status word comes with the first read


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_interpolate_launches_once_per_pass_level(ops, dtype, monkeypatch):
    r = fo.refine(*fo.box(), max_edge=0.3)
    parents, rng = r["parents"], np.random.default_rng(5)
    reads = Reads(monkeypatch)
    for shape in ((), (1,), (3,), (4,), (67,), (6, 3)):
        ops.calls.clear()
        reads.n = 0
        x = rng.standard_normal((8,) + shape).astype(dtype)
        got = meshprep.interpolate(x, parents)
        assert got.dtype == torch.from_numpy(x).dtype and np.array_equal(got.numpy(), fo.interpolate(x, parents))
        assert ops.calls == ["refine_interpolate"] * 3 and reads.n == 1
    ops.calls.clear()
    a, b = meshprep.interpolate([x, x], [parents[:8], parents[:26]])
    assert torch.equal(a, torch.from_numpy(x)) and tuple(b.shape) == (26, 6, 3) and ops.calls == ["refine_interpolate"]
    skin = np.abs(rng.standard_normal((8, 5)))
    skin /= skin.sum(1, keepdims=True)
    up = meshprep.interpolate(skin, parents).numpy()
    assert np.allclose(up.sum(1), 1.0) and np.array_equal(up[:8], skin)           # a convex combination stays one; [:V] carries it down
    for bad, text in ((parents[:5], "parents are integer"), (parents.astype(np.float64), "parents are integer"), (parents[:, :1], "parents are integer")):
        with pytest.raises(ValueError, match="interpolate: " + text):
            meshprep.interpolate(x, bad)
    with pytest.raises(ValueError, match="interpolate: values are float32 or float64"):
        meshprep.interpolate(np.arange(8), parents)
    for row, pair in ((30, (2, 30)), (30, (-1, 3)), (9, (100, 3))):
        wrong = parents.copy()
        wrong[row] = pair
        with pytest.raises(ValueError, match="interpolate: a parent is not a lower vertex"):
            meshprep.interpolate(x, wrong)
    with pytest.raises(ValueError, match="interpolate: one parents array per mesh"):
        meshprep.interpolate([x, x], [parents])


def test_prepare_mesh_refines_after_normalize_and_simplify_and_hands_the_refined_mesh_on(ops, monkeypatch):
    from morig_amd import geodesic, graph_build
    seen = {}
    monkeypatch.setattr(meshprep, "normalize", lambda verts: [(torch.as_tensor(np.asarray(v)) * 0.5, np.zeros(3), 0.5) for v in verts])

    def simplify(verts, faces, target_faces):
        seen["simplify"] = [tuple(v.shape) for v in verts]
        assert "refine_emit" not in ops.calls                                    # simplification comes first
        return [(v, torch.as_tensor(np.asarray(f))[:target_faces], torch.arange(len(v)), 4) for v, f in zip(verts, faces)]
    monkeypatch.setattr(meshprep, "simplify", simplify)
    monkeypatch.setattr(meshprep, "tpl_edges", lambda faces, n, self_loops: seen.setdefault("tpl", list(n)) and [None] * len(n))
    monkeypatch.setattr(meshprep, "sample_surface", lambda v, f, **kw: seen.setdefault("sampled", [torch.as_tensor(x) for x in f]) and ([None] * len(v), [None] * len(v)))
    monkeypatch.setattr(meshprep, "voxelize", lambda v, f, dims: seen.setdefault("vox", [tuple(x.shape) for x in v]) and [None] * len(v))
    monkeypatch.setattr(geodesic, "surface_geodesic_batched", lambda v, p, n: [None] * len(v))
    monkeypatch.setattr(graph_build, "get_geo_edges_from_distance", lambda *a: None)
    v, f = fo.box()
    want = fo.refine(v * 0.5, f, max_edge=0.2)                                   # lengths are those of the normalised frame
    d = meshprep.prepare_mesh(v, f, refine_max_edge=0.2)
    same_result((d["verts"], d["faces"], d["parents"], d["face_map"]), want)
    assert seen["tpl"] == [len(want["verts"])] and np.array_equal(seen["sampled"][0].numpy(), want["faces"]) and seen["vox"] == [want["verts"].shape]
    assert torch.equal(d["vertex_map"], torch.arange(8)) and d["scale"] == 0.5 and "simplify" not in seen
    seen.clear()
    ops.calls.clear()
    d = meshprep.prepare_mesh([v], [f], refine_min_verts=50, simplify_to=6)[0]
    want = fo.refine(v * 0.5, f[:6], min_verts=50)
    same_result((d["verts"], d["faces"], d["parents"], d["face_map"]), want)
    assert seen["simplify"] == [(8, 3)] and len(d["verts"]) == 50 and torch.equal(d["vertex_map"], torch.arange(8))
    wv = np.concatenate([v, v[:2]])                                              # two duplicates: clean's map composes, refinement moves no vertex
    d = meshprep.prepare_mesh(wv, f, clean=True, refine_max_edge=0.2)
    assert d["vertex_map"].tolist() == list(range(8)) + [0, 1] and len(d["verts"]) == len(fo.refine(v * 0.5, f, max_edge=0.2)["verts"])
    ops.calls.clear()
    d = meshprep.prepare_mesh(v, f)                                              # the default launches nothing new
    assert not ops.calls and "parents" not in d and "face_map" not in d and "faces" not in d


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_exports_are_typed_and_refuse_bad_arguments_without_a_device():
    names = [n for n in abi.SIGNATURES if n.startswith("morig_refine_")]
    order = list(abi.SIGNATURES)
    assert len(names) == 7 and set(names) <= set(native.EXPORTS)
    assert min(order.index(n) for n in names) > max(order.index(n) for n in order if n.startswith("morig_meshfix_"))   # appended behind them
    assert abi.CONSTANTS["MORIG_ABI_VERSION"] == 3 and len(abi.STRUCTS) == 8      # plain parameters: no new argument struct
    lib = native.load_library()
    K = abi.CONSTANTS
    for n in names:
        assert getattr(lib, n).argtypes is not None and hasattr(native.NativeOps, n[len("morig_"):])
    N = None
    calls = {                                                                     # name -> (arguments with a count of 4 everywhere, the count positions)
        "edge_records": ([N, 4, N, 4, N, N, 1, N, N, N, N, N, N], (1, 3, 6)),
        "mark": ([N, N, N, N, 4, N, 1, N, 1.0, N, N, N, N], (4, 6)),
        "budget": ([N, 4, N, N, 1, N, N], (1, 4)),
        "number": ([N, N, N, N, 4, N, N, 1, N, N], (4, 7)),
        "pattern": ([N, N, 4, N, N, N], (2,)),
        "emit": ([N, N, 4, N, N, N, N, 4, N, N, N, 1, N, N, N, 12, 4, 4, N, N, N, N, N], (2, 7, 11)),
        "interpolate": ([N, 8, 4, N, 2, 4, 4, N], (2, 6)),
    }
    assert set(calls) == {n[len("morig_refine_"):] for n in names}
    for name, (args, counts) in calls.items():
        fn = getattr(lib, "morig_refine_" + name)
        assert len(args) == len(abi.SIGNATURES["morig_refine_" + name][1]), name
        assert fn(*args) == K["MORIG_E_INVALID"], name                            # null pointers
        for at in counts:
            bad = list(args)
            bad[at] = -1
            assert fn(*bad) == K["MORIG_E_INVALID"], (name, at)                   # a negative count
    zeros = {"edge_records": [N, 0, N, 0, N, N, 0, N, N, N, N, N, N], "mark": [N, N, N, N, 0, N, 0, N, 1.0, N, N, N, N], "budget": [N, 0, N, N, 0, N, N],
             "number": [N, N, N, N, 0, N, N, 0, N, N], "pattern": [N, N, 0, N, N, N], "emit": [N, N, 0, N, N, N, N, 0, N, N, N, 0, N, N, N, 0, 0, 0, N, N, N, N, N],
             "interpolate": [N, 4, 0, N, 0, 0, 0, N]}
    for name, args in zeros.items():
        assert getattr(lib, "morig_refine_" + name)(*args) == K["MORIG_OK"], name  # nothing to do: before anything is launched
    too_many = (2 ** 31 - 257) // 3 + 1
    assert meshprep.REFINE_MAX_FACES == too_many - 1
    assert lib.morig_refine_edge_records(N, 4, N, too_many, N, N, 1, N, N, N, N, N, N) == K["MORIG_E_INVALID"]       # 3 F past the 32-bit rows
    assert lib.morig_refine_pattern(N, N, too_many, N, N, N) == K["MORIG_E_INVALID"]
    assert lib.morig_refine_emit(N, N, 4, N, N, N, N, 4, N, N, N, 1, N, N, N, 11, 4, 4, N, N, N, N, N) == K["MORIG_E_INVALID"]    # records != 3 F
    assert lib.morig_refine_emit(N, N, 4, N, N, N, N, 4, N, N, N, 1, N, N, N, 12, 3, 4, N, N, N, N, N) == K["MORIG_E_INVALID"]    # fewer rows out than in
    assert lib.morig_refine_emit(N, N, 4, N, N, N, N, 4, N, N, N, 1, N, N, N, 12, 4, 17, N, N, N, N, N) == K["MORIG_E_INVALID"]   # more than 4 children a face
    assert lib.morig_refine_mark(N, N, N, N, 2 ** 31 - 255, N, 1, N, 1.0, N, N, N, N) == K["MORIG_E_INVALID"]
    assert lib.morig_refine_interpolate(N, 2, 4, N, 0, 4, 4, N) == K["MORIG_E_INVALID"]                               # neither float nor double
    assert lib.morig_refine_interpolate(N, 4, 4, N, 3, 2, 4, N) == K["MORIG_E_INVALID"]                               # an empty range backwards
    assert lib.morig_refine_interpolate(N, 4, 4, N, 0, 5, 4, N) == K["MORIG_E_INVALID"]                               # rows past the end
    assert lib.morig_refine_interpolate(N, 8, 2 ** 40, N, 0, 4, 2 ** 40, N) == K["MORIG_E_INVALID"]                   # byte offsets past 63 bits
    assert (K["MORIG_REFINE_IDLE"], K["MORIG_REFINE_LENGTH"], K["MORIG_REFINE_LONGEST"]) == (0, 1, 2)
    prof = [lib.morig_prof_name(k) for k in range(K["MORIG_PROF_KINDS"])]
    at = prof.index(b"meshfix_fill")
    assert prof[at + 1:at + 4] == [b"refine_edges", b"refine_emit", b"refine_interpolate"]


# ------------------------------------------------------------------------------------------------------------------------- the host program
def test_split_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "refine_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "refine_host_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(17)
    # 8 masks x 3 listings x (the first diagonal shorter, the second shorter, a tie) x (the quad's old vertices ascending, descending)
    cases = []
    for mask, listing, x, ids in itertools.product(range(8), range(3), (1.0, -1.0, 0.0), ((10, 20, 30), (30, 20, 10), (20, 30, 10), (7, 5, 6))):
        marked = [c for c in range(3) if mask >> c & 1]
        apex = ([c for c in range(3) if c not in marked][0] + 2) % 3 if len(marked) == 2 else 0
        pos = np.zeros((3, 3))
        pos[apex], pos[(apex + 1) % 3], pos[(apex + 2) % 3] = (x, 4.0, 0.5), (-1.0, 0.0, 0.5), (1.0, 0.0, 0.5)
        t = [ids[c] for c in range(3)]
        mid = [100 + c if c in marked else -1 for c in range(3)]
        roll = lambda a: [a[(listing + c) % 3] for c in range(3)]
        cases.append((roll(t), roll(mid), np.array(roll(list(pos)))))
    pairs = np.concatenate([rng.standard_normal((60, 6)) * 10.0 ** rng.integers(-160, 150, (60, 1)),
                            [[0.0] * 6, [1, 2, 3, 1, 2, 3], [np.inf, 0, 0, 0, 0, 0], [np.nan, 0, 0, 1, 1, 1], [1e200, 0, 0, -1e200, 0, 0], [5e-324, 0, 0, 0, 0, 0],
                             [-0.0, 0, 0, 0.0, 0, 0]]])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("=q", len(cases)))
        for t, mid, pos in cases:
            fh.write(struct.pack("=6q", *t, *mid) + pos.astype(np.float64).tobytes())
        fh.write(struct.pack("=q", len(pairs)) + pairs.astype(np.float64).tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    raw, at = open(dst, "rb").read(), 0
    outcomes = set()
    for t, mid, pos in cases:
        head = struct.unpack_from("=4i", raw, at)
        kids = np.frombuffer(raw, dtype=np.int64, count=12, offset=at + 16).reshape(4, 3)
        at += 16 + 96
        new = {(min(t[c], t[(c + 1) % 3]), max(t[c], t[(c + 1) % 3])): mid[c] for c in range(3) if mid[c] >= 0}
        where = {t[c]: pos[c] for c in range(3)}
        where.update({m: fo.mid(where[e[0]], where[e[1]]) for e, m in new.items()})
        want = fo.split_face(t, new, where)
        assert head[0] == sum(1 << c for c in range(3) if mid[c] >= 0) and head[3] == len(want) == 1 + len(new)
        assert kids[:len(want)].tolist() == [list(k) for k in want] and (kids[len(want):] == -1).all(), (t, mid, kids, want)
        outcomes.add((len(new), head[2]))
    assert outcomes == {(0, 0), (1, 0), (2, 0), (2, 1), (3, 0)}
    with np.errstate(all="ignore"):
        for p in pairs:
            l0, l1, image = struct.unpack_from("=ddq", raw, at)
            m = struct.unpack_from("=3d", raw, at + 24)
            at += 48
            want = fo.sq(p[:3], p[3:])
            assert (l0 == want or (np.isnan(l0) and np.isnan(want))) and (l1 == l0 or np.isnan(l0))      # the direction does not matter
            assert image == (fe.bits(want) if np.isfinite(want) else -1) and image >= -1
            assert np.array_equal(np.array(m), np.array(fo.mid(p[:3], p[3:])), equal_nan=True)
    assert at == len(raw)
