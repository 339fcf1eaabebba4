"""GPU: ``morig_amd.meshprep.diagnose`` / ``clean`` / ``prepare_mesh(clean=True)`` (csrc/meshcheck.hip) against tests/topology_oracle.py.
Everything is compared with ``==`` / ``torch.equal``, nothing excused: the report, the labels, the round count of the component rule, the
component table with the bits of its areas (a component with a non-finite vertex has a NaN area on both sides: the payload of a NaN is
not compared), the boundary edge list and ``clean``'s four outputs. The sizes are those at which a kernel
takes another path or a run crosses a wave (64) or a workgroup (256). The round guard is exercised on the emulated ops only
(tests/test_topology_oracle.py), never provoked on the device."""
import functools
import itertools

import numpy as np
import pytest
import torch

import topology_oracle as to
from morig_amd import meshprep

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ("ascending", "descending", "zigzag", "random")
WELD_SIZES = (63, 64, 65, 255, 256, 257, 1025)


def lattice_mesh(n_verts, seed, special=True):
    """vertices on a 3 x 3 x 3 lattice (27 places: long runs of equal vertices anywhere in the sorted order), some of them -0.0, some rows
    not finite; random faces over them, so degenerate and duplicate faces abound"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-1, 2, (n_verts, 3)).astype(np.float64)
    v[rng.random((n_verts, 3)) < 0.3] *= -1.0                                    # 0.0 -> -0.0 among others
    if special:
        for k, x in enumerate((np.nan, np.inf, -np.inf, np.nan)):
            v[(7 * k + 3) % n_verts, k % 3] = x
        v[n_verts // 2] = v[(7 * 0 + 3) % n_verts]                               # a copy of a NaN row: still no weld
    f = rng.integers(0, n_verts, (2 * n_verts, 3))
    return v, f


def face_cases():
    v = np.random.default_rng(2).random((12, 3))
    f = [[0, 0, 1], [0, 1, 0], [1, 0, 0], [2, 2, 2]]                             # every position of a repeated corner
    f += [list(p) for p in itertools.permutations((3, 4, 5))]                    # duplicates in all six corner orders
    f += [[6, 7, 8]] + [[i % 9, (i + 1) % 9, 9 + i % 3] for i in range(300)] + [[8, 6, 7]]     # a duplicate pair 301 faces apart
    return v, np.array(f)


def interleaved():
    (va, fa), (vb, fb) = to.strip(40, "random", 1), to.strip(33, "zigzag")
    v, f = np.arange(240.0).reshape(80, 3) + 100.0, np.concatenate([2 * fa, 2 * fb + 1])   # even vertices one component, odd ones the other
    v[0:80:2], v[1:66:2] = va, vb + [0, 5, 0]
    return v, f                                                                  # vertices 67, 69 .. 79 are isolated


def soup(n):
    v = np.random.default_rng(4).random((3 * n, 3))
    return v, np.arange(3 * n).reshape(n, 3)


def last_edge_fan(k):
    v, f = to.fan(k, flip=(0,))
    return to.renumber(v, f, np.arange(len(v))[::-1].copy())                     # the fan's edge is the LAST key of the mesh


@functools.lru_cache(maxsize=None)
def cases():
    c = {f"weld_{n}": lattice_mesh(n, n) for n in WELD_SIZES}
    c["weld_all_coincident"] = (np.full((130, 3), 0.25), np.random.default_rng(0).integers(0, 130, (70, 3)))
    c["faces"] = face_cases()
    c["faces_all_degenerate"] = (np.random.default_rng(1).random((5, 3)), np.array([[0, 0, 1], [2, 3, 2], [4, 4, 4]]))
    c.update({f"fan_{k}": to.fan(k, flip=tuple(range(0, k, 3))) for k in (2, 3, 63, 64, 65, 257)})
    c.update({f"fan_last_{k}": last_edge_fan(k) for k in (2, 65, 257)})
    c["conflict_forward"], c["conflict_backward"] = to.fan(2), to.fan(2, flip=(0, 1))
    c.update({f"strip_{n}_{k}": to.strip(n, k, seed=n) for n in (65, 1025, 4096) for k in KINDS})
    c["interleaved"], c["soup_300"] = interleaved(), soup(300)
    c["cube"], c["split_cube"], c["torus"], c["mobius"] = to.cube(), to.split_cube(), to.torus(9, 7), to.mobius(13)
    c["tetrahedra"] = to.shared_edge_tetrahedra()
    return c


@functools.lru_cache(maxsize=None)
def want(name, weld=True):
    return to.diagnose(*cases()[name], weld)


def same(got, w):
    """one mesh's report (with components) against the oracle's"""
    for k in to.FIELDS + ("watertight", "rounds"):
        assert got[k] == w[k], (k, got[k], w[k])
    assert torch.equal(got["labels"].cpu(), torch.from_numpy(w["labels"][w["rep"]]))
    for k in ("root", "verts", "faces", "boundary_edges"):
        assert torch.equal(got["component_table"][k].cpu(), torch.from_numpy(w["component_table"][k])), k
    area = got["component_table"]["area"]
    assert area.dtype == torch.float64 and np.array_equal(area.cpu().numpy(), w["component_table"]["area"], equal_nan=True)   # a NaN is a NaN
    assert torch.equal(got["boundary_edge_list"].cpu(), torch.from_numpy(w["boundary_edge_list"]))


def run(names, weld=True):
    ms = [cases()[n] for n in names]
    return meshprep.diagnose([torch.from_numpy(m[0]).to(DEV) for m in ms], [m[1] for m in ms], weld=weld, return_components=True)


@pytest.mark.parametrize("name", sorted(cases()))
def test_a_mesh_alone_equals_the_oracle(name):
    same(run([name])[0], want(name))


@pytest.mark.parametrize("name", ["weld_257", "split_cube", "faces", "strip_65_random"])
def test_without_welding(name):
    same(run([name], weld=False)[0], want(name, False))


def test_known_answers_and_what_the_cases_hold():
    w = want
    assert w("cube")["euler"] == 2 and w("cube")["watertight"] and w("torus")["euler"] == 0 and w("torus")["watertight"]
    assert w("split_cube")["watertight"] and w("split_cube", False)["boundary_edges"] == 24
    assert w("mobius")["orientation_conflicts"] >= 1 and w("mobius")["nonmanifold_edges"] == 0 and w("tetrahedra")["nonmanifold_edges"] == 1
    assert w("conflict_forward")["orientation_conflicts"] == 1 == w("conflict_backward")["orientation_conflicts"]
    assert w("fan_257")["edge_table"][(0, 1)][0] == 257 and w("fan_last_257")["edge_table"][(257, 258)][0] == 257
    assert w("weld_all_coincident")["duplicate_verts"] == 129 and w("weld_all_coincident")["faces"] == 0
    assert w("weld_1025")["nonfinite_verts"] == 5 and w("weld_1025")["duplicate_verts"] > 900
    assert w("faces")["degenerate_faces"] == 4 and w("faces")["duplicate_faces"] >= 6 and w("faces")["surv"][-1] == 10
    assert w("faces_all_degenerate")["faces"] == 0 and w("faces_all_degenerate")["components"] == 0
    assert w("soup_300")["components"] == 300 and w("interleaved")["components"] == 2 and w("interleaved")["unreferenced_verts"] == 7


def test_equal_coordinates_in_two_meshes_of_a_batch_do_not_weld():
    v, f = cases()["split_cube"]
    reps = meshprep.diagnose([torch.from_numpy(v).to(DEV)] * 3, [f, f[:6], f])
    assert [r["duplicate_verts"] for r in reps] == [16, 16, 16] and [r["faces"] for r in reps] == [12, 6, 12]
    assert reps[0] == reps[2] and reps[0]["watertight"] and not reps[1]["watertight"]


def test_a_ragged_batch_equals_the_single_runs_and_a_second_run_bit_for_bit():
    names = sorted(cases())
    first, second = run(names), run(names)
    for n, a, b in zip(names, first, second):
        same(a, want(n))
        alone = run([n])[0]
        for other in (b, alone):
            assert {k: a[k] for k in to.FIELDS + ("watertight", "rounds")} == {k: other[k] for k in to.FIELDS + ("watertight", "rounds")}
            assert torch.equal(a["labels"], other["labels"]) and torch.equal(a["boundary_edge_list"], other["boundary_edge_list"])
            assert all(torch.equal(a["component_table"][k].view(torch.int64), other["component_table"][k].view(torch.int64)) for k in a["component_table"])


CLEAN_NAMES = ("weld_257", "faces", "interleaved", "soup_300", "split_cube", "faces_all_degenerate", "fan_65", "torus")


@pytest.mark.parametrize("keep", ["all", "largest", 1, 2, 40])
@pytest.mark.parametrize("drop", [True, False])
def test_clean_equals_the_oracle_and_is_idempotent(keep, drop):
    ms = [cases()[n] for n in CLEAN_NAMES]
    out, reports = meshprep.clean([torch.from_numpy(m[0]).to(DEV) for m in ms], [m[1] for m in ms], keep=keep, drop_unreferenced=drop,
                                  return_report=True)
    bits = lambda x: x.view(torch.int64) if x.is_floating_point() else x          # coordinates are copied: equal bit for bit, NaN included
    for n, (v, f), o, r in zip(CLEAN_NAMES, ms, out, reports):
        w = to.clean(v, f, True, keep, drop)
        for x, y in zip(o, w):
            assert x.is_cuda and torch.equal(bits(x.cpu()), bits(torch.from_numpy(y))), n
        assert all(r[k] == want(n)[k] for k in to.FIELDS)
    again = meshprep.clean([o[0] for o in out], [o[1] for o in out], drop_unreferenced=drop)
    for o, a in zip(out, again):
        assert torch.equal(bits(a[0]), bits(o[0])) and torch.equal(a[1], o[1])
        assert torch.equal(a[2].cpu(), torch.arange(len(o[0]))) and torch.equal(a[3].cpu(), torch.arange(len(o[1])))


def one_ring_components(edge_index, n):
    e = edge_index.cpu().numpy()
    return len(set(to.union_find_labels(n, zip(e[0].tolist(), e[1].tolist())).tolist()))


def test_prepare_mesh_clean_feeds_a_connected_one_ring_and_a_solid_interior():
    v, f = cases()["split_cube"]
    kw = dict(n_samples=64, oversample=2, dims=16, self_loops=False)
    raw, fixed = meshprep.prepare_mesh(v, f, **kw), meshprep.prepare_mesh(v, f, clean=True, **kw)
    assert one_ring_components(raw["tpl_edge_index"], 24) == 6 and "report" not in raw            # seams: six patches
    assert fixed["verts"].shape == (8, 3) and one_ring_components(fixed["tpl_edge_index"], 8) == 1
    assert fixed["report"]["duplicate_verts"] == 16 and fixed["report"]["watertight"]
    assert torch.equal(fixed["vertex_map"].cpu(), torch.from_numpy(to.clean(v, f)[2])) and fixed["faces"].shape == (12, 3)
    assert fixed["vox"].data[8, 8, 8] and fixed["vox"].data.all()                                 # a solid cube fills its grid
    holed = meshprep.prepare_mesh(v, f[2:], clean=True, **kw)                                     # one side missing: the fill leaks
    assert holed["report"]["boundary_edges"] == 4 and not holed["report"]["watertight"]
    assert not holed["vox"].data[8, 8, 8] and holed["vox"].data.any()                             # the shell only
    tv, tf = cases()["torus"]                                                                     # every vertex twice, the faces alternate between the copies
    tv2, tf2 = np.concatenate([tv, tv]), tf + (np.arange(len(tf)) % 2 * len(tv))[:, None]
    both = meshprep.prepare_mesh(tv2, tf2, clean=True, simplify_to=40, **kw)
    vm = both["vertex_map"].cpu()
    assert both["report"]["duplicate_verts"] == len(tv) and both["report"]["watertight"] and 0 < both["faces"].shape[0] <= 40
    assert vm.shape == (2 * len(tv),) and (vm >= 0).all() and int(vm.max()) < both["verts"].shape[0] and torch.equal(vm[:len(tv)], vm[len(tv):])
