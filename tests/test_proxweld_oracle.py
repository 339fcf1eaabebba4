"""CPU: the oracle of the tolerance weld (tests/proxweld_oracle.py: brute force, no grid) on answers known by hand; the host logic of
``morig_amd.meshprep.diagnose`` / ``clean`` / ``repair`` / ``prepare_mesh`` with ``weld_tol`` on an emulated op layer
(tests/proxweld_emulate.py through ``runtime._test_ops``) against that oracle; the new exports' typing and refusals through the C ABI; and
csrc/proxweld_core.h as the stand-alone program tools/proxweld_host_check.cpp, built with the address and undefined-behaviour sanitizers
and run as a program (never loaded into Python). Every comparison is exact."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import proxweld_emulate as pe
import proxweld_oracle as po
import repair_oracle as ro
import topology_oracle as to
from morig_amd import abi, meshprep, native, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E3, F3 = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)


@pytest.fixture()
def ops():
    emu = pe.ProxweldRepairOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def damaged():
    """exact duplicates next to near ones, -0.0, a NaN row, an infinite row and a far vertex, with faces over them"""
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0.0, 0.0], [1 + 1e-9, 0, 0], [0, 1, 1e-9], [np.nan, 0, 0], [np.inf, 1, 1], [1, 0, 0],
                  [5, 5, 5], [1 - 1e-9, 1e-9, 0], [0, 0, 1], [0, 1e-9, 1]])
    f = np.array([[0, 1, 2], [3, 4, 5], [0, 8, 11], [3, 10, 12], [6, 7, 9], [2, 5, 9], [0, 3, 9]])
    return v, f


def cases():
    return [("seam_cube", *po.seam_cube(), 1e-8), ("seam_torus", *po.seam_torus(10, 6), 1e-8), ("chain", *po.chain(40, 0.9e-3), 1e-3),
            ("clusters", *po.clusters(5, 6, 0.5e-4), 1e-4), ("damaged", *damaged(), 1e-8), ("damaged_exact", *damaged(), 0.0),
            ("cube_wide", *po.seam_cube(), 2.0), ("empty", E3, F3, 1e-3), ("all_nan", np.full((4, 3), np.nan), np.array([[0, 1, 2], [1, 2, 3]]), 1e-3)]


def exact_generators():
    out = [to.cube(), to.split_cube(), to.torus(8, 6), to.mobius(), to.shared_edge_tetrahedra(), to.fan(7, flip=(2, 5)), damaged()]
    out += [to.strip(n, k, seed=n) for n in (65, 257) for k in ("ascending", "random")]
    return out


# ------------------------------------------------------------------------------------------------------------------------- known answers
def test_the_jittered_seam_cube_falls_apart_exactly_and_welds_at_1e_8():
    v, f = po.seam_cube()
    assert np.abs(v - to.split_cube()[0]).max() <= 1e-9
    e = to.diagnose(v, f)
    assert (e["components"], e["boundary_edges"], e["duplicate_verts"], e["watertight"]) == (6, 24, 0, False)
    w = po.diagnose(v, f, 1e-8)
    assert (w["components"], w["watertight"], w["euler"], w["duplicate_verts"], w["weld_links"], w["near_verts"]) == (1, True, 2, 16, 24, 16)
    assert 0.0 < w["weld_spread"] <= 1e-8 and w["weld_tol"] == 1e-8


def test_a_chain_welds_into_one_class_whose_spread_says_so():
    eps = 2.0 ** -10
    v, f = po.chain(200, 0.9 * eps)
    w = po.weld(v, eps)
    assert set(w["rep"].tolist()) == {0} and w["near_verts"] == 199 and w["weld_links"] == 199
    far = 199 * (0.9 * eps)
    assert w["weld_spread"] == math.sqrt(far * far) and w["weld_spread"] > eps and round(w["weld_spread"] / eps, 6) == 179.1
    assert po.weld(v, 0.8 * eps)["near_verts"] == 0


def test_a_tolerance_of_zero_is_the_exact_weld_on_every_generator():
    for v, f in exact_generators():
        got, want = po.diagnose(v, f, 0.0), to.diagnose(v, f)
        assert all(got[k] == want[k] for k in to.FIELDS + ("watertight", "rounds")) and np.array_equal(got["rep"], want["rep"])
        assert (got["near_verts"], got["weld_links"], got["weld_spread"]) == (0, 0, 0.0)
        for x, y in zip(po.clean(v, f, 0.0), to.clean(v, f)):
            assert x.tobytes() == y.tobytes()


def test_cleaning_is_idempotent_under_an_absolute_tolerance():
    v, f = po.seam_torus(12, 12, strips=4)
    assert to.diagnose(v, f)["components"] == 4
    cv, cf, vmap, fmap = po.clean(v, f, 1e-8)
    assert len(cv) == 144 and po.diagnose(v, f, 1e-8)["watertight"] and po.diagnose(v, f, 1e-8)["euler"] == 0
    again = po.weld(cv, 1e-8)
    assert again["weld_links"] == 0 and again["near_verts"] == 0
    for name, v, f, eps in cases():
        cv, cf = po.clean(v, f, eps)[:2]
        assert po.weld(cv, eps)["weld_links"] == 0, name                          # two representatives are farther apart than the tolerance
        c2 = po.clean(cv, cf, eps)
        assert c2[0].tobytes() == cv.tobytes() and np.array_equal(c2[1], cf) and np.array_equal(c2[2], np.arange(len(cv))), name


def test_a_tolerance_whose_square_is_no_normal_double_links_nothing():
    assert po.EPS2_MIN == 2.0 ** -1022 and (2.0 ** -511) ** 2 == po.EPS2_MIN and 0.0 < 1.4e-154 ** 2 < po.EPS2_MIN
    for eps in (0.0, 1e-170, 1e-162, 1e-160, 1.4e-154):
        v = po.subnormal_square(eps) if eps else np.array([[0.0, 0, 0], [5e-324, 0, 0], [1e-200, 0, 0]])
        assert po.weld(v, eps)["weld_links"] == 0
        assert po.weld(po.border_pairs(eps, eps * (1 + 2.0 ** -20), 0.0, 1000.0 * eps), eps)["weld_links"] == 0
    # with the comparison alone the first case would link (1, 2), two cells apart: what the rule is there to exclude
    v = po.subnormal_square(1e-160)
    assert po.len2(v[1], v[2]) <= np.float64(1e-160) * np.float64(1e-160) and v[2, 0] - v[1, 0] > 1e-160 * (1 + 2.0 ** -20)
    for eps in (2.0 ** -511, 1.5e-154, 1e-150):
        assert po.weld(po.subnormal_square(eps), eps)["links"] == [(0, 1)]       # a normal square: the pair inside the tolerance, no other
        assert po.weld(po.border_pairs(eps, eps * (1 + 2.0 ** -20), 0.0, 1000.0 * eps), eps)["weld_links"] >= 27


def test_a_vertex_that_is_not_finite_never_welds_and_exact_classes_follow_their_node():
    v, f = damaged()
    w = po.weld(v, 1e-8)
    assert w["rep"].tolist() == [0, 1, 2, 0, 1, 2, 6, 7, 1, 9, 1, 11, 11] and w["rep0"].tolist() == [0, 1, 2, 0, 4, 5, 6, 7, 1, 9, 10, 11, 12]
    assert (w["near_verts"], w["weld_links"]) == (4, 5)                           # 1 - 4, 1 - 10, 4 - 10, 2 - 5, 11 - 12


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


def same_bits(a, b):
    """torch.equal, NaN rows included"""
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


def same_report(got, want):
    for k in to.FIELDS + ("watertight", "rounds") + po.WELD_FIELDS:
        kind = bool if k == "watertight" else float if k in ("weld_tol", "weld_spread") else int
        assert got[k] == want[k] and type(got[k]) is kind, (k, got[k], want[k])
    assert tuple(got)[:len(to.FIELDS)] == meshprep.REPORT_FIELDS == to.FIELDS and meshprep.WELD_FIELDS == po.WELD_FIELDS


def test_diagnose_with_per_mesh_tolerances_equals_the_oracle(ops):
    cs = cases()
    reps = meshprep.diagnose([c[1] for c in cs], [c[2] for c in cs], weld_tol=[c[3] for c in cs], return_components=True)
    for (name, v, f, eps), r in zip(cs, reps):
        w = po.diagnose(v, f, eps)
        same_report(r, w)
        for k in ("root", "verts", "faces", "boundary_edges", "area"):
            assert np.array_equal(r["component_table"][k].numpy(), w["component_table"][k], equal_nan=k == "area"), (name, k)   # a NaN face has a NaN area
        assert np.array_equal(r["boundary_edge_list"].numpy(), w["boundary_edge_list"]), name
    alone = meshprep.diagnose([cs[1][1]], [cs[1][2]], weld_tol=cs[1][3])[0]       # a mesh alone: what it gives in the batch
    assert alone == {k: x for k, x in reps[1].items() if k in alone}
    plain = meshprep.diagnose([cs[0][1]], [cs[0][2]])[0]
    assert not set(po.WELD_FIELDS) & set(plain) and plain["components"] == 6      # without a tolerance the report is the one it was
    one = meshprep.diagnose([c[1] for c in cs[:2]], [c[2] for c in cs[:2]], weld_tol=1e-8)
    assert [r["weld_tol"] for r in one] == [1e-8, 1e-8] and one[0]["watertight"]


@pytest.mark.parametrize("keep", ["all", "largest", 3])
@pytest.mark.parametrize("drop", [True, False])
def test_clean_with_a_tolerance_equals_the_oracle_and_is_idempotent(ops, keep, drop):
    cs = cases()
    out, reports = meshprep.clean([c[1] for c in cs], [c[2] for c in cs], weld_tol=[c[3] for c in cs], keep=keep, drop_unreferenced=drop,
                                  return_report=True)
    for (name, v, f, eps), o, r in zip(cs, out, reports):
        for x, y in zip(o, po.clean(v, f, eps, keep, drop)):
            assert x.dtype == (torch.float64 if x.is_floating_point() else torch.int64) and x.numpy().tobytes() == y.tobytes(), name
        same_report(r, po.diagnose(v, f, eps))
        again, rep = meshprep.clean([o[0]], [o[1]], weld_tol=eps, drop_unreferenced=drop, return_report=True)
        assert same_bits(again[0][0], o[0]) and torch.equal(again[0][1], o[1]) and torch.equal(again[0][2], torch.arange(len(o[0])))
        assert rep[0]["weld_links"] == 0 and rep[0]["near_verts"] == 0 and rep[0]["weld_spread"] == 0.0


def test_a_tolerance_of_zero_gives_the_bits_of_the_exact_weld(ops):
    ms = exact_generators()[:7]
    a = meshprep.clean([m[0] for m in ms], [m[1] for m in ms], weld_tol=0)
    b = meshprep.clean([m[0] for m in ms], [m[1] for m in ms])
    for x, y in zip(a, b):
        assert all(same_bits(p, q) for p, q in zip(x, y))


def test_repair_with_a_tolerance_closes_the_seam_cube(ops):
    v, f = po.seam_cube()
    out, reports = meshprep.repair([v, v], [f, f], fill_holes="all", weld_tol=[1e-8, 0.0], return_report=True)
    for o, r, eps in zip(out, reports, (1e-8, 0.0)):
        want = ro.repair(po.moved(v, eps)[0], f, fill_holes="all")
        for x, k in zip(o, ("verts", "faces", "vertex_map", "face_map", "flipped")):
            assert x.numpy().tobytes() == want[k].tobytes(), k
        same_report(r["input"], po.diagnose(v, f, eps))
        assert all(r[k] == want["report"][k] for k in meshprep.REPAIR_FIELDS)
    assert (reports[0]["filled_loops"], reports[0]["closed_components"], len(out[0][0])) == (0, 1, 8)
    assert reports[1]["filled_loops"] == 6                                        # the exact weld fans six "holes"


def test_relative_tolerances_use_the_box_of_the_finite_vertices(ops, monkeypatch):
    (sv, sf), (dv, df) = po.seam_cube(), damaged()
    sv = sv * 10.0                                                               # the jitter grows with the mesh, and so does the tolerance
    reads = Reads(monkeypatch)
    reps = meshprep.diagnose([sv, dv, E3, np.full((2, 3), np.nan)], [sf, df, F3, F3], weld_tol=[1e-8, 1e-9, 0.5, 0.5], weld_tol_rel=True)
    assert ops.calls.count("mesh_bbox") == 1
    for (v, f, t), r in zip(((sv, sf, 1e-8), (dv, df, 1e-9), (E3, F3, 0.5), (np.full((2, 3), np.nan), F3, 0.5)), reps):
        eps = t * po.diagonal(v)
        assert r["weld_tol"] == eps
        same_report(r, po.diagnose(v, f, eps))
    assert reps[0]["watertight"] and reps[2]["weld_tol"] == 0.0 and reps[1]["weld_tol"] == 1e-9 * math.sqrt(75.0)   # the far vertex at (5, 5, 5)


def test_max_links_refuses_before_anything_is_emitted(ops):
    v, f = po.seam_cube()
    with pytest.raises(ValueError, match=r"clean: weld_tol 1e-08 of mesh 1 is too large for this mesh: more than max_links = 30 links"):
        meshprep.clean([v, v], [f, f], weld_tol=1e-8, max_links=30)
    assert "proxweld_emit_links" not in ops.calls and "meshcheck_face_keys" not in ops.calls
    with pytest.raises(ValueError, match="repair: weld_tol 1e-08 of mesh 0 is too large for this mesh: more than max_links = 5 links"):
        meshprep.repair([v], [f], weld_tol=1e-8, max_links=5)
    with pytest.raises(ValueError, match="diagnose: weld_tol 2.0 of mesh 0 is too large"):
        meshprep.diagnose([v], [f], weld_tol=2.0, max_links=275)                   # one cell, all 24 x 23 / 2 pairs linked
    assert meshprep.diagnose([v], [f], weld_tol=2.0, max_links=276)[0]["weld_links"] == 276


def test_error_texts(ops):
    v, f = po.seam_cube()
    for kw, text in ((dict(weld_tol=-1e-9), r"weld_tol -1e-09 of mesh 0: a non-negative finite number"), (dict(weld_tol=[0.0, np.nan]), "weld_tol nan of mesh 1"),
                     (dict(weld_tol=[np.inf, 0.0]), "weld_tol inf of mesh 0"), (dict(weld_tol=[1e-3]), r"weld_tol: one tolerance, or one per mesh \(2\), not 1"),
                     (dict(weld_tol=True), "weld_tol True of mesh 0"), (dict(weld_tol="small"), "weld_tol 'small' of mesh 0"),
                     (dict(weld_tol=1e-3, weld=False), "weld_tol needs weld=True"), (dict(weld_tol_rel=True), "weld_tol_rel needs a weld_tol"),
                     (dict(max_links=5), "max_links needs a weld_tol"), (dict(weld_tol=1e-3, max_links=-1), "max_links -1: a number of links")):
        for fn in (meshprep.diagnose, meshprep.clean, meshprep.repair):
            with pytest.raises(ValueError, match=fn.__name__ + ": " + text):          # the function that was called is the one named
                fn([v, v], [f, f], **kw)
    with pytest.raises(ValueError, match="diagnose: weld_tol of mesh 0: the tolerance times the bounding-box diagonal is not finite"):
        meshprep.diagnose([v * 1e300], [f], weld_tol=1e300, weld_tol_rel=True)
    assert [c for c in ops.calls if c not in ("meshcheck_coord_keys", "meshcheck_weld_mark", "meshcheck_run_rep", "mesh_bbox")] == []


EXACT_CALLS = ["meshcheck_coord_keys", "meshcheck_weld_mark", "meshcheck_run_rep", "meshcheck_face_keys", "meshcheck_face_mark", "meshcheck_run_rep",
               "meshcheck_face_edges", "meshcheck_cc_round", "meshcheck_edge_classify"]


def test_the_call_list_with_a_tolerance_and_the_call_list_of_today_without(ops, monkeypatch):
    v, f = po.seam_cube()
    reads = Reads(monkeypatch)
    r = meshprep.diagnose([v], [f])[0]
    rounds = ops.calls.count("meshcheck_cc_round")
    assert [c for c in ops.calls if c != "meshcheck_cc_round"] == [c for c in EXACT_CALLS if c != "meshcheck_cc_round"]
    assert ops.calls.index("meshcheck_cc_round") == 7 and rounds == r["rounds"] and reads.n == rounds + 1
    ops.calls.clear()
    reads.n = 0
    r = meshprep.diagnose([v], [f], weld_tol=1e-8)[0]
    weld = ["proxweld_cell_keys", "proxweld_count_links", "proxweld_emit_links"]
    at = ops.calls.index("proxweld_spread")
    link_rounds = ops.calls[:at].count("meshcheck_cc_round")
    assert ops.calls[:at + 1] == EXACT_CALLS[:3] + weld + ["meshcheck_cc_round"] * link_rounds + ["proxweld_spread"]
    assert [c for c in ops.calls[at + 1:] if c != "meshcheck_cc_round"] == [c for c in EXACT_CALLS[3:] if c != "meshcheck_cc_round"]
    # ONE added read (the links to allocate) next to the rounds of the second component loop; the report still comes with one read
    assert reads.n == 1 + link_rounds + r["rounds"] + 1 and link_rounds >= 2
    ops.calls.clear()
    meshprep.clean([v], [f])
    assert ops.calls[:7] == EXACT_CALLS[:7] and ops.calls[-2:] == ["meshcheck_keep_flags", "meshcheck_compact"] and not [c for c in ops.calls if "proxweld" in c]


def test_prepare_mesh_hands_the_tolerance_to_its_clean_or_repair_step_only_when_it_is_set(ops, monkeypatch):
    from morig_amd import geodesic, graph_build
    seen = {}
    monkeypatch.setattr(meshprep, "normalize", lambda verts: [(torch.as_tensor(v), np.zeros(3), 1.0) for v in verts])
    monkeypatch.setattr(meshprep, "tpl_edges", lambda faces, n, self_loops: seen.setdefault("tpl", list(n)) and [None] * len(n))
    monkeypatch.setattr(meshprep, "sample_surface", lambda v, f, **kw: ([None] * len(v), [None] * len(v)))
    monkeypatch.setattr(meshprep, "voxelize", lambda v, f, dims: [None] * len(v))
    monkeypatch.setattr(geodesic, "surface_geodesic_batched", lambda v, p, n: [None] * len(v))
    monkeypatch.setattr(graph_build, "get_geo_edges_from_distance", lambda *a: None)
    v, f = po.seam_cube()
    d = meshprep.prepare_mesh(v, f, repair=True, weld_tol=1e-8)
    want = ro.repair(po.moved(v, 1e-8)[0], f, fill_holes="all")
    assert d["verts"].numpy().tobytes() == want["verts"].tobytes() and np.array_equal(d["faces"].numpy(), want["faces"]) and seen.pop("tpl") == [8]
    assert d["report"]["input"]["weld_links"] == 24 and d["report"]["closed_components"] == 1
    d = meshprep.prepare_mesh([v * 4.0], [f], clean=True, weld_tol=1e-8, weld_tol_rel=True)[0]
    assert d["report"]["watertight"] and d["report"]["weld_tol"] == 1e-8 * po.diagonal(v * 4.0) and seen.pop("tpl") == [8]
    with pytest.raises(ValueError, match="prepare_mesh: weld_tol belongs to the clean / repair step"):
        meshprep.prepare_mesh(v, f, weld_tol=1e-8)
    # without a tolerance the two steps are called as they always were: stubs of the old signatures
    real_clean, real_repair = meshprep._clean_meshes, meshprep._repair_meshes

    def old_clean(verts, faces, return_report):
        return real_clean(verts, faces, return_report=return_report)

    def old_repair(verts, faces, fill_holes, return_report):
        return real_repair(verts, faces, fill_holes=fill_holes, return_report=return_report)
    monkeypatch.setattr(meshprep, "_clean_meshes", old_clean)
    monkeypatch.setattr(meshprep, "_repair_meshes", old_repair)
    assert meshprep.prepare_mesh(v, f, clean=True)["report"]["components"] == 6 and seen.pop("tpl") == [24]
    assert meshprep.prepare_mesh(v, f, repair=True)["report"]["filled_loops"] == 6
    monkeypatch.setattr(meshprep, "clean", lambda verts, faces, weld, keep, return_report: real_clean(verts, faces, weld=weld, keep=keep, return_report=True))
    assert len(meshprep.repair([v], [f])[0][0]) == 24                             # repair calls clean as it always did


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_exports_are_typed_and_refuse_bad_arguments_without_a_device():
    names = [n for n in abi.SIGNATURES if n.startswith("morig_proxweld_")]
    order = list(abi.SIGNATURES)
    assert len(names) == 4 and set(names) <= set(native.EXPORTS)
    assert min(order.index(n) for n in names) > max(order.index(n) for n in order if n.startswith("morig_refine_"))    # appended behind them
    assert abi.CONSTANTS["MORIG_ABI_VERSION"] == 3 and len(abi.STRUCTS) == 8      # plain parameters: no new argument struct
    lib = native.load_library()
    K = abi.CONSTANTS
    for n in names:
        assert getattr(lib, n).argtypes is not None and hasattr(native.NativeOps, n[len("morig_"):])
    N = None
    calls = {                                                                     # name -> (arguments with a count of 4 everywhere, the count positions)
        "cell_keys": ([N, N, N, 4, N, 1, N, N, N, N, N], (3, 5)),
        "count_links": ([N, N, N, 4, N, 1, N, N, N], (3, 5)),
        "emit_links": ([N, N, N, 4, N, 1, N, N, N, 4, N, N], (3, 5, 9)),
        "spread": ([N, N, N, 4, N, 1, N, N], (3, 5)),
    }
    assert set(calls) == {n[len("morig_proxweld_"):] for n in names}
    for name, (args, counts) in calls.items():
        fn = getattr(lib, "morig_proxweld_" + name)
        assert len(args) == len(abi.SIGNATURES["morig_proxweld_" + name][1]), name
        assert fn(*args) == K["MORIG_E_INVALID"], name                            # null pointers
        for at in counts:
            bad = list(args)
            bad[at] = -1
            assert fn(*bad) == K["MORIG_E_INVALID"], (name, at)                   # a negative count
            big = list(args)
            big[at] = 2 ** 31 - 255 if at != 5 else 2 ** 31 - 1
            if not (name == "emit_links" and at == 9) and not (at == 5 and name != "cell_keys"):
                assert fn(*big) == K["MORIG_E_INVALID"], (name, at)               # past the 32-bit rows
    assert lib.morig_proxweld_emit_links(N, N, N, 4, N, 1, N, N, N, 2 ** 31 - 255, N, N) == K["MORIG_E_INVALID"]
    zeros = {"cell_keys": [N, N, N, 4, N, 0, N, N, N, N, N], "count_links": [N, N, N, 0, N, 1, N, N, N], "emit_links": [N, N, N, 4, N, 1, N, N, N, 0, N, N],
             "spread": [N, N, N, 4, N, 0, N, N]}
    for name, args in zeros.items():
        assert getattr(lib, "morig_proxweld_" + name)(*args) == K["MORIG_OK"], name   # nothing to do: before anything is launched
    prof = [lib.morig_prof_name(k) for k in range(K["MORIG_PROF_KINDS"])]
    at = prof.index(b"refine_interpolate")
    assert prof[at + 1:at + 4] == [b"proxweld_keys", b"proxweld_links", b"proxweld_spread"] and K["MORIG_PROF_KINDS"] == 96


# ------------------------------------------------------------------------------------------------------------------------- the host program
def host_cases():
    rng = np.random.default_rng(23)
    out = []
    for eps in (0.25, 1e-3, 3.0, 1e-12):                                          # the tolerance sets the cell: partners across all 26 borders
        h = pe.cell_side(eps, 1000.0 * eps)
        assert h == eps * (1.0 + 2.0 ** -20)
        out += [(po.border_pairs(eps, h, frac, 1000.0 * eps), eps) for frac in (0.0, 0.9)]
    for extent in (1000.0, 1e-3):                                                 # the clamp of h: the extent sets the cell, eight tolerances wide
        h = pe.cell_side(0.0, extent)
        assert h == extent * 2.0 ** -20
        out += [(po.border_pairs(h / 8.0, h, frac, extent), h / 8.0) for frac in (0.0, 1.0 - 1.0 / 16.0)]
    special = np.array([[0.0, 0, 0], [-0.0, -0.0, -0.0], [1e-150, 0, 0], [0, 1e-150, 1e-150], [np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0],
                        [1e-150, 1e-150, 0], [5e-324, 0, 0], [0, 0, 2e-150]])
    out += [(special, 1e-150), (special, 1.5e-150), (special, 0.0), (special, 1e-170), (special * 1e300, 1e150), (special * 1e300 + 1e150, 1.5e150)]
    # a squared tolerance that is 0 or subnormal links nothing (below 2^-511 = 1.49e-154); the smallest normal square links as any other
    out += [(po.subnormal_square(eps), eps) for eps in (1e-162, 1e-160, 1e-157, 1.4e-154, 2.0 ** -511, 1.5e-154)]
    for eps in (1e-160, 1.4e-154, 2.0 ** -511, 1.6e-154):
        out += [(po.border_pairs(eps, pe.cell_side(eps, 1000.0 * eps), frac, 1000.0 * eps), eps) for frac in (0.0, 0.9)]
    out += [(np.array([[1e150, -1e150, 0], [1e150, -1e150, 1e140], [-1e150, 1e150, 0], [np.nan, np.nan, np.nan]]), 1e141)]
    out += [(np.zeros((5, 3)), 1e-3), (np.zeros((0, 3)), 1.0), (np.array([[1.0, 2, 3]]), 0.5), (np.array([[0.0, 0, 0], [0.25, 0, 0]]), 0.25),
            (np.array([[0.0, 0, 0], [0.25 * (1 + 2.0 ** -52), 0, 0]]), 0.25), (np.array([[0.0, 0, 0], [0.1875, 0.25, 0]]), 0.3125),
            (np.array([[0.0, 0, 7], [1, 0, 7], [0.5, 1e-9, 7], [0.5, 0, 7]]), 1e-8)]
    for _ in range(12):                                                           # random clouds with partners near the threshold
        eps = 10.0 ** rng.uniform(-12, 0.5)
        base = rng.uniform(-1, 1, (40, 3)) * 10.0 ** rng.uniform(-3, 3)
        d = rng.standard_normal((40, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append((np.concatenate([base, base + d * eps * rng.choice([0.5, 1.0, 1.0 - 1e-15, 1.0 + 1e-15, 1.5], (40, 1))]), eps))
    return out


def test_proxweld_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "proxweld_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "proxweld_host_check.cpp"), "-o", exe], check=True)
    cs = host_cases()
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("=q", len(cs)))
        for v, eps in cs:
            fh.write(struct.pack("=qd", len(v), eps) + np.ascontiguousarray(v, dtype=np.float64).tobytes())
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    raw, at, linked, crossed = open(dst, "rb").read(), 0, 0, 0
    for n_case, (v, eps) in enumerate(cs):
        v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
        frame = np.frombuffer(raw, dtype=np.float64, count=4, offset=at)
        cells = np.frombuffer(raw, dtype=np.int64, count=3 * len(v), offset=at + 32).reshape(-1, 3)
        at += 32 + 24 * len(v)
        n_links, = struct.unpack_from("=q", raw, at)
        links = np.frombuffer(raw, dtype=np.int64, count=2 * n_links, offset=at + 8).reshape(-1, 2)
        at += 8 + 16 * n_links
        fin = np.isfinite(v).all(1)
        lo = v[fin].min(0) + 0.0 if fin.any() else np.zeros(3)
        with np.errstate(all="ignore"):
            extent = float((v[fin].max(0) - lo).max()) if fin.any() else 0.0
        want_frame = np.array([*lo, pe.cell_side(eps, extent)])
        assert frame.tobytes() == want_frame.tobytes(), (n_case, frame, want_frame)
        want_cells = np.array([[pe.cell_coord(x, l, want_frame[3]) for x, l in zip(p, lo)] if ok else [-1, -1, -1] for p, ok in zip(v, fin)],
                              dtype=np.int64).reshape(-1, 3)
        assert np.array_equal(cells, want_cells), n_case
        want = po.links_of(v, np.nonzero(fin)[0], eps)                           # the brute force: no grid
        assert [tuple(l) for l in links.tolist()] == want, (n_case, eps)
        linked += len(want)
        crossed += sum(1 for a, b in want if (cells[a] != cells[b]).any())
    assert at == len(raw) and linked > 400 and crossed > 250                     # the borders were crossed, not only approached
