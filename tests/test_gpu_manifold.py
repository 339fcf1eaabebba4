"""GPU: ``morig_amd.meshprep.split_nonmanifold`` / ``repair(split=True)`` / ``prepare_mesh(split=True)`` (csrc/meshsplit.hip) against
tests/manifold_oracle.py. Everything is compared with ``==`` / ``torch.equal``, nothing excused: vertices by their bits where they are no
NaN (a NaN is a NaN on both sides), faces, both maps, ``source``, every field of the report, ``split_rounds`` included. One ragged batch
of all cases per parametrisation. The sizes are those at which a kernel can go wrong: a fan whose corners fill less than a wave, a wave
(64), a workgroup (256) and more, as a path and as a cycle (a cycle has at least three faces: two faces around a centre that share both
rim edges are duplicates of each other), the centre on the lowest, the highest and a random index; many fans on ONE vertex (the
minimum and the count land on one word); runs of records and fans that lie across a workgroup boundary."""
import functools

import numpy as np
import pytest
import torch

import manifold_oracle as mo
import repair_oracle as ro
import topology_oracle as to
from morig_amd import meshprep

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
CENTRES = ("lowest", "highest", "random")


def flipped_at_random(mesh, seed, share=0.3):
    v, f = mesh
    rng = np.random.default_rng(seed)
    return v, ro.flip_faces(f, np.nonzero(rng.random(len(f)) < share)[0])


def with_values(mesh, rows, value):
    v, f = mesh
    v = v.copy()
    for r, c in rows:
        v[r, c] = value
    return v, f


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for i, n in enumerate(SIZES):
        for centre in (CENTRES if n in (65, 257) else (CENTRES[i % 3],)):
            c[f"path_{n}_{centre}"] = mo.disc(n, False, centre, seed=n)
            if n >= 3:
                c[f"cycle_{n}_{centre}"] = mo.disc(n, True, centre, seed=n + 1)
    for i, k in enumerate((2, 3, 64, 65, 257)):
        c[f"cones_{k}"] = mo.cones(k, apex=CENTRES[i % 3], seed=k)
    for k in (3, 64, 65, 200):
        c[f"fan_{k}"] = to.fan(k, flip=tuple(range(1, k, 3)))
    c["link_across_a_workgroup"] = mo.padded(to.fan(2, flip=(1,)), 85)           # the two-run holds sorted records 255 and 256
    c["fan_200_across_a_workgroup"] = mo.padded(to.fan(200, flip=(5, 150)), 52)  # the run of 200 begins at 156
    c["corners_across_a_workgroup"] = mo.padded(mo.disc(6, closed=True), 84)     # the centre's corners are nodes 252, 255, 258, ...
    c["tetrahedra"] = to.shared_edge_tetrahedra()
    c["tetrahedra_flipped"] = (to.shared_edge_tetrahedra()[0], ro.flip_faces(to.shared_edge_tetrahedra()[1], (1, 5, 6)))
    c["bowtie"], c["touching_holes"], c["fin"] = ro.bowtie(), ro.cube_two_holes_touching(), mo.cube_with_fin()
    c["pinched_torus"], c["corner_cubes"], c["box"] = mo.pinched_torus(), mo.cubes_at_a_corner(), mo.folded_bowtie_box()
    c["moebius"], c["cube"], c["torus"] = to.mobius(), ro.cube(), to.torus(6, 5)
    for n, name in enumerate(("bowtie", "fin", "pinched_torus", "corner_cubes", "cones_65", "cycle_257_random", "box")):
        c[name + "_flipped_at_random"] = flipped_at_random(c[name], 40 + n)
    c["raw"] = (np.concatenate([mo.cube_with_fin()[0], ro.cube()[0][:2], [[9.0, 9, 9]]]),      # a duplicate and a degenerate face, dropped by the clean first
                np.concatenate([mo.cube_with_fin()[1], [[9, 10, 3], [0, 0, 1], ro.cube()[1][5][[1, 2, 0]]]]))
    c["apex_nan"] = with_values(mo.cones(3), [(0, 0)], np.nan)
    c["apex_negative_zero"] = with_values(mo.cones(3), [(0, 0), (0, 1)], -0.0)
    c["pinch_nan_and_negative_zero"] = with_values(ro.bowtie(), [(5, 0), (5, 2)], np.nan)
    c["pinch_nan_and_negative_zero"] = with_values(c["pinch_nan_and_negative_zero"], [(5, 1)], -0.0)
    c["no_faces"] = (np.random.default_rng(0).random((5, 3)), np.zeros((0, 3), dtype=np.int64))
    c["nothing"] = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    return c


@functools.lru_cache(maxsize=None)
def oracle(name):
    return mo.split(*cases()[name])


@functools.lru_cache(maxsize=None)
def oracle_repair(name):
    return mo.repair_split(*cases()[name], fill_holes="all")


@functools.lru_cache(maxsize=None)
def device(names):
    out, reports = meshprep.split_nonmanifold([cases()[n][0] for n in names], [cases()[n][1] for n in names], return_report=True)
    torch.cuda.synchronize()
    return dict(zip(names, zip(out, reports)))


@functools.lru_cache(maxsize=None)
def device_repair(names):
    out, reports = meshprep.repair([cases()[n][0] for n in names], [cases()[n][1] for n in names], fill_holes="all", return_report=True, split=True)
    torch.cuda.synchronize()
    return dict(zip(names, zip(out, reports)))


def same_verts(v, want, what):
    gv = v.cpu().numpy()
    assert v.dtype == torch.float64 and gv.shape == want.shape and np.array_equal(np.isnan(gv), np.isnan(want)), what
    assert gv[~np.isnan(gv)].tobytes() == want[~np.isnan(want)].tobytes(), what


def same(got, want, report=None, what=""):
    v, f, vm, fm, src = got
    same_verts(v, want["verts"], what)
    for x, k in ((f, "faces"), (vm, "vertex_map"), (fm, "face_map"), (src, "source")):
        assert x.dtype == torch.int64 and x.is_cuda and tuple(x.shape) == want[k].shape and np.array_equal(x.cpu().numpy(), want[k]), (what, k)
    if report is not None:
        for k in mo.FIELDS + ("split_rounds",):
            assert report[k] == want["report"][k] and type(report[k]) is int, (what, k, report[k], want["report"][k])
        for k in to.FIELDS + ("rounds", "watertight"):
            assert report["input"][k] == want["report"]["input"][k], (what, k)


def test_the_cases_sit_where_the_kernels_change_blocks():
    clean = lambda n: to.clean(*cases()[n])[1]
    assert mo.run_at(clean("link_across_a_workgroup"), 255, 256) == (255, 2)
    at, n = mo.run_at(clean("fan_200_across_a_workgroup"), 156, 157)
    assert n == 200 and at < 256 < at + n
    cf = clean("corners_across_a_workgroup")
    assert [3 * i + list(t).index(252) for i, t in enumerate(cf) if 252 in t] == [252, 255, 258, 261, 264, 267]
    rep = {n: oracle(n)["report"] for n in cases()}
    assert all(rep[f"fan_{k}"]["max_fans"] == k and rep[f"fan_{k}"]["added_verts"] == 2 * (k - 1) for k in (3, 64, 65, 200))
    assert all(rep[f"cones_{k}"]["max_fans"] == k and rep[f"cones_{k}"]["added_verts"] == k - 1 for k in (2, 3, 64, 65, 257))
    assert all(r["added_verts"] == 0 and r["max_fans"] == 1 for n, r in rep.items() if n.startswith(("path_", "cycle_")))
    assert rep["path_1025_" + CENTRES[8 % 3]]["split_rounds"] >= 4 and rep["raw"]["input"]["duplicate_faces"] == 2 and rep["raw"]["input"]["degenerate_faces"] == 1 and rep["raw"]["added_verts"] == 2
    assert rep["moebius"]["added_verts"] == 0 and rep["tetrahedra"]["added_verts"] == 2 and rep["pinch_nan_and_negative_zero"]["added_verts"] == 1
    v = oracle("pinch_nan_and_negative_zero")["verts"]
    assert np.isnan(v[-1, 0]) and np.signbit(v[-1, 1]) and v[-1, 1] == 0


def test_the_ragged_batch_equals_the_oracle():
    got = device(tuple(cases()))
    for name in cases():
        o, r = got[name]
        same(o, oracle(name), r, name)
    assert meshprep.split_nonmanifold([], []) == [] and meshprep.split_nonmanifold([], [], return_report=True) == ([], [])
    (v, f, _, _, _), _ = got["tetrahedra"]
    d = meshprep.diagnose([v], [f], weld=False)[0]
    assert d["watertight"] and d["components"] == 2 and meshprep.diagnose([v], [f])[0]["nonmanifold_edges"] == 1     # and the trap: the weld rejoins them


def test_repair_with_split_equals_the_oracle_and_leaves_nothing_tangled():
    names = tuple(cases())
    got = device_repair(names)
    for name in names:
        o, r = got[name]
        want = oracle_repair(name)
        assert len(o) == 6
        same_verts(o[0], want["verts"], name)
        for x, k in zip(o[1:], ("faces", "vertex_map", "face_map", "flipped", "source")):
            assert np.array_equal(x.cpu().numpy(), want[k]) and x.dtype == (torch.bool if k == "flipped" else torch.int64), (name, k)
        for k in ro.FIELDS + ("orient_rounds",):
            assert r[k] == want["report"][k] and type(r[k]) is int, (name, k, r[k], want["report"][k])
        assert r["split"] == want["report"]["split"] and list(r["split"]) == list(meshprep.SPLIT_FIELDS) + ["split_rounds"], name
        if r["nonorientable_components"] == 0:
            assert r["tangled_boundary_edges"] == 0, name
    closed = [n for n in names if got[n][1]["nonorientable_components"] == 0 and len(got[n][0][1])]
    after = meshprep.diagnose([got[n][0][0] for n in closed], [got[n][0][1] for n in closed], weld=False)
    assert all(d["watertight"] for d in after), [n for n, d in zip(closed, after) if not d["watertight"]]
    assert len(closed) == len(names) - 3 and got["bowtie"][1]["filled_loops"] == got["touching_holes"][1]["filled_loops"] == 1
    assert got["tetrahedra"][1]["closed_components"] == 2


def test_repair_without_split_gives_what_it_gave():
    names = tuple(cases())
    out, reports = meshprep.repair([cases()[n][0] for n in names], [cases()[n][1] for n in names], fill_holes="all", return_report=True, split=False)
    for n, o, r in zip(names, out, reports):
        want = ro.repair(*cases()[n], fill_holes="all")
        assert len(o) == 5 and list(r) == list(ro.FIELDS) + ["orient_rounds", "input"], n
        same_verts(o[0], want["verts"], n)
        for x, k in zip(o[1:], ("faces", "vertex_map", "face_map", "flipped")):
            assert np.array_equal(x.cpu().numpy(), want[k]), (n, k)
        assert all(r[k] == want["report"][k] for k in ro.FIELDS + ("orient_rounds",)), n
    assert reports[names.index("bowtie")]["tangled_boundary_edges"] == 16 and reports[names.index("touching_holes")]["tangled_boundary_edges"] == 6


def test_a_mesh_alone_gives_the_bits_it_gives_in_the_batch():
    batch = device(tuple(cases()))
    for name, (v, f) in cases().items():
        (alone,), (report,) = meshprep.split_nonmanifold([v], [f], return_report=True)
        for x, y in zip(alone, batch[name][0]):
            assert x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name
        assert report == batch[name][1], name


def test_a_second_run_gives_the_same_bits_and_a_second_application_is_the_identity():
    names = tuple(cases())
    first = device(names)
    out, reports = meshprep.split_nonmanifold([cases()[n][0] for n in names], [cases()[n][1] for n in names], return_report=True)
    for n, o, r in zip(names, out, reports):
        assert r == first[n][1] and all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(o, first[n][0])), n
    got, reps = meshprep.split_nonmanifold([first[n][0][0] for n in names], [first[n][0][1] for n in names], weld=False, return_report=True)
    for n, o, r in zip(names, got, reps):
        a = first[n][0]
        assert r["added_verts"] == 0 and r["nonmanifold_edges"] == 0 and r["max_fans"] <= 1, n
        assert torch.equal(o[1], a[1]) and o[0].cpu().numpy().tobytes() == a[0].cpu().numpy().tobytes(), n
        ident = torch.arange(len(a[0]), device=o[2].device)
        assert torch.equal(o[2], ident) and torch.equal(o[4], ident) and torch.equal(o[3], torch.arange(len(a[1]), device=o[3].device)), n


def test_prepare_mesh_with_split_gives_a_solid_grid_where_repair_alone_gives_the_shell():
    v, f = mo.folded_bowtie_box()
    kw = dict(n_samples=64, oversample=2, dims=16, self_loops=False)
    shell, solid = meshprep.prepare_mesh(v, f, repair=True, **kw), meshprep.prepare_mesh(v, f, repair=True, split=True, **kw)
    assert shell["report"]["tangled_boundary_edges"] == 8 and shell["report"]["filled_loops"] == 0 and "source" not in shell
    assert not shell["vox"].data[8, 8, 8] and shell["vox"].data.any()            # the shell only: two holes that touch are never fanned
    assert solid["vox"].data[8, 8, 8] and solid["vox"].data.all()                # solid
    want = mo.repair_split(v, f, fill_holes="all")
    assert np.array_equal(solid["faces"].cpu().numpy(), want["faces"]) and np.array_equal(solid["source"].cpu().numpy(), want["source"])
    assert np.array_equal(solid["vertex_map"].cpu().numpy(), want["vertex_map"]) and solid["report"]["split"] == want["report"]["split"]
    assert (solid["report"]["filled_loops"], solid["report"]["tangled_boundary_edges"], solid["report"]["split"]["added_verts"]) == (1, 0, 1)
    only = meshprep.prepare_mesh(v, f, clean=True, split=True, **kw)
    assert np.array_equal(only["faces"].cpu().numpy(), mo.split(v, f)["faces"]) and only["report"]["added_verts"] == 1 and "flipped" not in only
    with pytest.raises(ValueError, match="prepare_mesh: split belongs to the clean / repair step"):
        meshprep.prepare_mesh(v, f, split=True, **kw)
