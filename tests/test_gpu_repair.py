"""GPU: ``morig_amd.meshprep.repair`` / ``prepare_mesh(repair=True)`` (csrc/meshfix.hip) against tests/repair_oracle.py. Everything is
compared with ``==`` / ``torch.equal``, nothing excused: vertices with the bits of the centroids (a NaN is a NaN on both sides: its payload
is not compared), faces, both maps, ``flipped`` and every field of the report, ``orient_rounds`` included. The sizes are those at which a
kernel takes another path or a run crosses a wave (64) or a workgroup (256). A CLOSED component has an even number of faces (3 F = 2 E),
so the closed components whose sum needs the fold have 12, 64 and 66 faces; the odd sizes are tori with one face taken out."""
import functools

import numpy as np
import pytest
import torch

import repair_oracle as ro
import topology_oracle as to
from morig_amd import meshprep

pytestmark = pytest.mark.gpu

KINDS = ("ascending", "descending", "zigzag", "random")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
LOOPS = (3, 4, 63, 64, 65, 129)


def flipped_at_random(mesh, seed, share=0.3):
    v, f = mesh
    rng = np.random.default_rng(seed)
    return v, ro.flip_faces(f, np.nonzero(rng.random(len(f)) < share)[0])


def torus_of(n_faces):
    """a torus of ``n_faces`` faces: closed where the count is even, with face 5 taken out where it is odd"""
    n, m = {64: (4, 8), 66: (3, 11), 256: (8, 16), 258: (3, 43), 1026: (19, 27)}[n_faces + n_faces % 2]
    v, f = to.torus(n, m)
    return (v, f) if n_faces % 2 == 0 else (v, ro.drop_faces(f, [5]))


def soup(n):
    v = np.random.default_rng(4).random((3 * n, 3))
    return v, np.arange(3 * n).reshape(n, 3)


def fan_with_neighbours(k=200):
    """k faces on one edge (a run of k records that links nothing), every second of them linked to a face of its own across its edge
    (1, 2 + i), some of those traversing it the wrong way"""
    v, f = to.fan(k, flip=tuple(range(0, k, 7)))
    extra_v = [[1.5, 2.0 + i, 0.5] for i in range(0, k, 2)]
    extra_f = [(1, len(v) + j, 2 + i) if j % 3 else (len(v) + j, 1, 2 + i) for j, i in enumerate(range(0, k, 2))]
    return np.concatenate([v, extra_v]), np.concatenate([f, np.array(extra_f, dtype=np.int64)])


def padded(mesh, n_loose):
    """``n_loose`` loose triangles on lower vertex numbers in front of ``mesh``: its first sorted record lies at 3 n_loose"""
    (sv, sf), (v, f) = soup(n_loose), mesh
    return np.concatenate([sv + 10.0, v]), np.concatenate([sf, f + len(sv)])


def two_discs():
    v, f = to.torus(9, 8)
    return v, ro.drop_faces(f, [0, 1, 16, 17, 70, 71, 87])                       # loops of 6 and 5, apart


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
        kinds = KINDS if n in (65, 257) else (KINDS[i % 4],)
        for k in kinds:
            c[f"strip_{n}_{k}"] = flipped_at_random(to.strip(n + 2, k, seed=n), 100 + n)
    for n in SIZES[2:]:
        c[f"torus_{n}"] = flipped_at_random(torus_of(n), 200 + n)
    c["cube"] = (ro.cube()[0], ro.flip_faces(ro.cube()[1], (1, 4, 7, 10)))
    c["cube_inverted"] = (ro.cube()[0], ro.flip_faces(ro.cube()[1], range(12)))
    for n in (64, 66):
        c[f"closed_{n}_inverted"] = (torus_of(n)[0], ro.flip_faces(torus_of(n)[1], range(n)))
        c[f"closed_{n}_mostly_inverted"] = (torus_of(n)[0], ro.flip_faces(torus_of(n)[1], range(3, n)))
    c["fan_200"] = fan_with_neighbours()
    c["fan_200_across_a_workgroup"] = padded(fan_with_neighbours(), 84)           # the run of 200 holds sorted records 252 .. 451
    c["link_across_a_workgroup"] = padded(flipped_at_random(ro.cube(), 7, 0.4), 85)       # the first link holds records 255 and 256
    c["boundary_across_a_workgroup"] = padded(to.strip(5), 85)
    c["soup_300"] = soup(300)
    c["moebius"] = to.mobius()
    c["moebius_64"] = to.mobius(64)
    c["tetrahedra"] = (to.shared_edge_tetrahedra()[0], ro.flip_faces(to.shared_edge_tetrahedra()[1], (1, 5, 6)))
    for L in LOOPS:
        q = max(0, (L - 2 - L % 2) // 2)
        c[f"loop_{L}"] = flipped_at_random(ro.torus_disc(max(6, q + 3), 4, L), 300 + L, 0.05)
    c["two_loops"] = flipped_at_random(two_discs(), 9, 0.1)
    c["bowtie"] = ro.bowtie()
    c["touching_holes"] = ro.cube_two_holes_touching()
    c["cube_nan_volume"] = with_values((ro.cube()[0], ro.flip_faces(ro.cube()[1], (2, 9))), [(7, 1)], np.nan)   # S is a NaN: the majority decides
    c["loop_nan_centroid"] = with_values(ro.torus_disc(6, 4, 5), [(0, 2)], np.nan)
    c["loop_negative_zero"] = with_values((ro.cube()[0], ro.cube()[1][2:]), [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2)], -0.0)
    c["raw"] = (np.concatenate([ro.cube()[0], ro.cube()[0][:2], [[9.0, 9, 9]]]),
                np.concatenate([ro.flip_faces(ro.cube()[1][2:], (3,)), [[8, 9, 3], [0, 0, 1], ro.cube()[1][5][[1, 2, 0]]]]))
    c["no_faces"] = (np.random.default_rng(0).random((5, 3)), np.zeros((0, 3), dtype=np.int64))
    c["nothing"] = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    return c


LOOPED = tuple(f"loop_{L}" for L in LOOPS) + ("two_loops", "raw", "bowtie", "loop_negative_zero")


@functools.lru_cache(maxsize=None)
def oracle(name, orient=True, fill=None):
    return ro.repair(*cases()[name], orient=orient, fill_holes=fill)


@functools.lru_cache(maxsize=None)
def device(names, orient=True, fill=None):
    out, reports = meshprep.repair([cases()[n][0] for n in names], [cases()[n][1] for n in names], orient=orient, fill_holes=fill, return_report=True)
    torch.cuda.synchronize()
    return dict(zip(names, zip(out, reports)))


def same(got, want, report=None, what=""):
    v, f, vm, fm, fl = (x.cpu() for x in got)
    assert v.dtype == torch.float64 and f.dtype == vm.dtype == fm.dtype == torch.int64 and fl.dtype == torch.bool, what
    gv, wv = v.numpy(), want["verts"]
    assert gv.shape == wv.shape and np.array_equal(np.isnan(gv), np.isnan(wv)) and gv[~np.isnan(gv)].tobytes() == wv[~np.isnan(wv)].tobytes(), what
    for x, k in ((f, "faces"), (vm, "vertex_map"), (fm, "face_map"), (fl, "flipped")):
        assert np.array_equal(x.numpy(), want[k]), (what, k)
    if report is not None:
        for k in ro.FIELDS + ("orient_rounds",):
            assert report[k] == want["report"][k] and type(report[k]) is int, (what, k, report[k], want["report"][k])
        for k in to.FIELDS + ("rounds", "watertight"):
            assert report["input"][k] == want["report"]["input"][k], (what, k)


def test_the_cases_reach_the_kernels_edges():
    rep = {n: oracle(n, True, "all")["report"] for n in cases()}
    assert rep["cube_inverted"]["inverted_components"] == 1 and rep["cube_inverted"]["flipped_faces"] == 12
    for n in (64, 66):                                                           # whichever way the generator winds its torus
        assert rep[f"closed_{n}_inverted"]["flipped_faces"] in (0, n) and rep[f"closed_{n}_mostly_inverted"]["flipped_faces"] in (3, n - 3)
        assert rep[f"closed_{n}_inverted"]["inverted_components"] + ro.repair(*torus_of(n))["report"]["inverted_components"] == 1
        assert rep[f"closed_{n}_inverted"]["closed_components"] == 1
    assert rep["soup_300"]["orientation_components"] == 300 and rep["soup_300"]["flipped_faces"] == 0 and rep["soup_300"]["filled_loops"] == 300
    assert rep["moebius"]["nonorientable_components"] == rep["moebius_64"]["nonorientable_components"] == 1
    assert [len(list(oracle(f"loop_{L}", True, "all")["loops"].values())[0]) for L in LOOPS] == list(LOOPS)
    assert sorted(map(len, oracle("two_loops", True, "all")["loops"].values())) == [5, 6]
    assert rep["bowtie"]["tangled_boundary_edges"] == 16 and rep["touching_holes"]["tangled_boundary_edges"] == 6
    assert rep["fan_200"]["input"]["nonmanifold_edges"] == 1 and rep["fan_200"]["orientation_components"] == 200 and rep["fan_200"]["flipped_faces"] > 0
    assert rep["cube_nan_volume"]["closed_components"] == 1 and rep["cube_nan_volume"]["flipped_faces"] == 2 and rep["cube_nan_volume"]["inverted_components"] == 0
    assert np.isnan(oracle("loop_nan_centroid", True, "all")["centroids"][0, 2]) and not np.isnan(oracle("loop_nan_centroid", True, "all")["centroids"][0, :2]).any()
    assert all(1 <= rep[n]["flipped_faces"] < len(cases()[n][1]) for n in cases() if n.startswith(("strip_6", "strip_25", "strip_1025", "torus_")))
    for name, at in (("fan_200_across_a_workgroup", 252), ("link_across_a_workgroup", 255), ("boundary_across_a_workgroup", 255)):
        keys = sorted((lo << 32) | hi for (lo, hi), r in ro.edge_table(cases()[name][1]).items() for _ in r)
        assert keys[at - 1] != keys[at] and keys[at] == keys[at + 1] if "boundary" not in name else keys[at - 1] != keys[at] != keys[at + 1], name
        assert at < 256 <= at + (200 if "fan" in name else 2 if "link" in name else 1)


@pytest.mark.parametrize("orient,fill", [(True, None), (True, "all"), (False, "all")])
def test_the_ragged_batch_equals_the_oracle(orient, fill):
    got = device(tuple(cases()), orient, fill)
    for name in cases():
        o, r = got[name]
        same(o, oracle(name, orient, fill), r, name)
    assert meshprep.repair([], []) == []


@pytest.mark.parametrize("fill", [3, 4, 5, 62, 63, 64, 65, 66, 128, 129, 130])
def test_fill_holes_by_length_equals_the_oracle(fill):
    got = device(LOOPED, True, fill)
    filled = 0
    for name in LOOPED:
        o, r = got[name]
        same(o, oracle(name, True, fill), r, name)
        filled += r["filled_loops"]
    print(f"fill_holes = {fill}: {filled} loops filled")
    assert filled == sum(1 for n in LOOPED for l in oracle(n)["loops"].values() if len(l) <= fill)


@pytest.mark.parametrize("name", list(cases()))
def test_a_mesh_alone_gives_the_bits_it_gives_in_the_batch(name):
    v, f = cases()[name]
    (alone,), (report,) = meshprep.repair([v], [f], fill_holes="all", return_report=True)
    batched, batched_report = device(tuple(cases()), True, "all")[name]
    for x, y in zip(alone, batched):
        assert x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert report == batched_report


def test_a_second_run_gives_the_same_bits_and_a_second_application_changes_nothing():
    names = tuple(cases())
    first = device(names, True, "all")
    out, reports = meshprep.repair([cases()[n][0] for n in names], [cases()[n][1] for n in names], fill_holes="all", return_report=True)
    for n, o, r in zip(names, out, reports):
        assert r == first[n][1] and all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(o, first[n][0])), n
    # idempotence, where the volume rule does not meet a component that a fill has just closed facing inward, and no coordinate is a NaN
    # (NaN rows never weld, so they repair to themselves too; they are left out only because the comparison below is ``torch.equal``)
    again = [n for n in names if not n.startswith(("loop_nan", "cube_nan"))]
    got = meshprep.repair([first[n][0][0] for n in again], [first[n][0][1] for n in again], fill_holes="all", return_report=True)
    for n, o, r in zip(again, *got):
        want = ro.repair(first[n][0][0].cpu().numpy(), first[n][0][1].cpu().numpy(), fill_holes="all")
        same(o, want, r, n)
        if want["report"]["flipped_faces"] == 0:
            assert torch.equal(o[0], first[n][0][0]) and torch.equal(o[1], first[n][0][1]) and not o[4].any(), n
            assert torch.equal(o[2].cpu(), torch.arange(len(o[0]))) and torch.equal(o[3].cpu(), torch.arange(len(o[1]))) and r["added_faces"] == 0, n
    turned = [n for n, o, r in zip(again, *got) if r["flipped_faces"]]
    print("closed by the fill and judged by volume on the second application:", turned)
    assert all(first[n][1]["filled_loops"] > 0 for n in turned)


def test_filled_meshes_are_watertight_and_every_loop_raises_euler_by_one():
    got = device(tuple(cases()), True, "all")
    for name in tuple(f"loop_{L}" for L in LOOPS) + ("two_loops", "raw", "torus_63", "torus_1025"):
        (v, f, _, _, _), r = got[name]
        if np.isnan(cases()[name][0]).any():
            continue
        after = meshprep.diagnose([v], [f])[0]
        assert after["watertight"] and after["euler"] == r["input"]["euler"] + r["filled_loops"] and r["filled_loops"] == r["boundary_loops"] >= 1, name
        assert after["orientation_conflicts"] == 0 and r["tangled_boundary_edges"] == 0


def test_prepare_mesh_repair_gives_a_solid_grid_and_outward_normals():
    v, f = ro.cube()
    f = ro.flip_faces(f[2:], (4,))                                               # one side missing, one face the wrong way round
    kw = dict(n_samples=64, oversample=2, dims=16, self_loops=False)
    holed, fixed = meshprep.prepare_mesh(v, f, clean=True, **kw), meshprep.prepare_mesh(v, f, repair=True, **kw)
    assert not holed["vox"].data[8, 8, 8] and holed["vox"].data.any()            # the shell only
    assert fixed["vox"].data[8, 8, 8] and fixed["vox"].data.all()                # solid
    rep = fixed["report"]
    assert (rep["flipped_faces"], rep["filled_loops"], rep["added_faces"], rep["input"]["orientation_conflicts"]) == (1, 1, 4, 3)
    assert fixed["verts"].shape == (9, 3) and fixed["faces"].shape == (14, 3) and fixed["flipped"].sum() == 1 and bool(fixed["flipped"][4])
    want = ro.repair(v, f, fill_holes="all")
    assert np.array_equal(fixed["faces"].cpu().numpy(), want["faces"]) and np.array_equal(fixed["vertex_map"].cpu().numpy(), want["vertex_map"])
    # the normalised cube is [-0.5, 0.5] x [0, 1] x [-0.5, 0.5]: an outward normal n at a surface point p has n . (p - centre) = 0.5
    centre = torch.tensor([0.0, 0.5, 0.0], dtype=torch.float64)
    side = lambda d: ((d["normals"].cpu() * (d["samples"].cpu() - centre)).sum(1))
    assert torch.allclose(side(fixed), torch.full((64,), 0.5, dtype=torch.float64), atol=1e-12)
    print("samples of the cleaned, unrepaired mesh on a reversed face:", int((side(holed) < 0).sum()), "of 64")
