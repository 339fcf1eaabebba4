"""GPU: ``morig_amd.meshprep.refine`` / ``interpolate`` / ``prepare_mesh(refine_max_edge=)`` (csrc/refine.hip) against
tests/refine_oracle.py. Everything is compared with ``==`` / ``torch.equal``, nothing excused: vertices by their bits (a NaN is a NaN on both
sides: its payload is not compared), faces, parents, the face map and every field of the report. The sizes are those at which a run of
records crosses a wave (64) or a workgroup (256); the limits are chosen so that about half the edges of a pass are marked."""
import functools

import numpy as np
import pytest
import torch

import refine_oracle as fo
import topology_oracle as to
from morig_amd import meshprep

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)


def same(got, want, report=None):
    v, f, p, m = got
    assert v.dtype == torch.float64 and f.dtype == p.dtype == m.dtype == torch.int64 and v.is_cuda
    gv, wv = v.cpu().numpy(), want["verts"]
    assert gv.shape == wv.shape and np.array_equal(np.isnan(gv), np.isnan(wv))
    assert np.array_equal(np.where(np.isnan(gv), 0.0, gv).view(np.int64), np.where(np.isnan(wv), 0.0, wv).view(np.int64))
    for x, k in ((f, "faces"), (p, "parents"), (m, "face_map")):
        assert np.array_equal(x.cpu().numpy(), want[k]), k
    if report is not None:
        assert report == want["report"], (report, want["report"])
        assert all(type(report[k]) is int for k in ("passes", "verts", "faces", "faces_kept", "degenerate_kept")) and type(report["converged"]) is bool


def check(mesh, **kw):
    v, f = mesh
    want = fo.refine(v, f, **kw)
    got, report = meshprep.refine(v, f, return_report=True, **kw)
    print({k: report[k] for k in ("passes", "edges_split", "verts", "faces", "converged", "stalled")})
    same(got, want, report)
    return want


def triangle(l0, l1, l2):
    """corners with |v0 v1| = l0, |v1 v2| = l1, |v2 v0| = l2"""
    x = (l0 * l0 + l2 * l2 - l1 * l1) / (2 * l0)
    return np.array([[0.0, 0, 0], [l0, 0, 0], [x, np.sqrt(l2 * l2 - x * x), 0]])


def soup(triangles, rotations):
    """separate triangles as one mesh, triangle k listed from corner rotations[k]"""
    v = np.concatenate([t + np.array([3.0 * k, 0, 0]) for k, t in enumerate(triangles)])
    f = np.array([[3 * k + (r + c) % 3 for c in range(3)] for k, r in enumerate(rotations)], dtype=np.int64)
    return v, f


def all_patterns():
    """the 8 masks x 3 listings: a marked edge is 1.5, 1.6 or 1.7 long, an unmarked one 1.0, 1.05 or 1.1 (the limit is 1.3; no two
    sides are equal, so no diagonal is a tie)"""
    tris, rots = [], []
    for mask in range(8):
        for r in range(3):
            tris.append(triangle(*[1.5 + 0.1 * c if mask >> c & 1 else 1.0 + 0.05 * c for c in range(3)]))
            rots.append(r)
    return soup(tris, rots)


def tie_mesh():
    """two marked edges and a quad whose diagonals are exactly equal: triangles (b, c, a) listed from every corner, as (0, 1, 2) -- the old
    vertices of the quad ascend along the unmarked edge -- and as (1, 0, 2), where they descend"""
    tri = np.array([[-1.0, 0, 0], [1.0, 0, 0], [0.0, 4, 0]])
    v = np.concatenate([tri + np.array([4.0 * k, 0, 0]) for k in range(6)])
    f = np.array([[3 * k + (0, 1, 2)[(r + c) % 3] for c in range(3)] for k, r in enumerate(range(3))] +
                 [[3 * k + (1, 0, 2)[(r + c) % 3] for c in range(3)] for k, r in zip(range(3, 6), range(3))], dtype=np.int64)
    return v, f


@functools.lru_cache(maxsize=None)
def sized(n):
    return fo.patch(n, seed=n)


# ------------------------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", SIZES)
def test_max_edge_at_the_sizes_where_runs_cross_a_wave_and_a_workgroup(n):
    want = check(sized(n), max_edge=0.9)
    first = want["report"]["edges_split"][0]
    assert first > 0 and (n < 63 or first < len(fo.edge_classes(sized(n)[1])))      # some edges of the first pass are marked, some are not


@pytest.mark.parametrize("n", SIZES)
def test_min_verts_at_the_same_sizes(n):
    want = check(sized(n), min_verts=2 * (n + 2) + 5)
    assert want["report"]["verts"] == 2 * (n + 2) + 5 and want["report"]["converged"]


@pytest.mark.parametrize("n", (65, 257))
def test_both_modes_one_after_the_other(n):
    want = check(sized(n), max_edge=1.1, min_verts=3 * n)
    assert want["report"]["verts"] >= 3 * n


# ------------------------------------------------------------------------------------------------------------------------- patterns
def test_every_pattern_in_every_listing():
    mesh = all_patterns()
    want = check(mesh, max_edge=1.3, max_passes=1)
    r = want["report"]
    assert (r["faces_kept"], r["faces_split_1"], r["faces_split_2"], r["faces_split_3"]) == (3, 9, 9, 3)
    # the outcome does not depend on the corner a face lists first: the three listings of a mask give the same triangles in space
    for k in range(0, 24, 3):
        shapes = []
        for j in range(k, k + 3):
            mine = want["verts"][want["faces"][want["face_map"] == j]] - np.array([3.0 * j, 0, 0])
            shapes.append({frozenset(tuple(np.round(p, 9)) for p in t) for t in mine})
        assert shapes[0] == shapes[1] == shapes[2] and len(shapes[0]) == 1 + bin(k // 3).count("1")


def test_the_diagonal_tie_goes_to_the_lower_old_vertex():
    mesh = tie_mesh()
    want = check(mesh, max_edge=3.0, max_passes=1)
    assert want["report"]["faces_split_2"] == 6
    v, f = want["verts"], want["faces"]
    for k in range(6):
        quad = f[want["face_map"] == k][1:]                                       # the two triangles of the quad share its diagonal
        diagonal = sorted(set(quad[0].tolist()) & set(quad[1].tolist()))
        old = sorted(x for x in set(quad.reshape(-1).tolist()) if x < len(mesh[0]))
        assert len(diagonal) == 2 and diagonal[0] == old[0]                       # through the LOWER of the two old vertices
        other = sorted(set(quad.reshape(-1).tolist()) - set(diagonal))
        assert fo.sq(v[diagonal[0]], v[diagonal[1]]) == fo.sq(v[other[0]], v[other[1]])   # and it was a tie


def test_a_fan_of_200_faces_on_one_marked_edge():
    v, f = to.fan(200, flip=tuple(range(0, 200, 7)))
    want = check((v, f), max_edge=0.95, max_passes=2)
    assert want["history"][0][1][0] == (0, 1) and (want["faces"] == len(v)).sum() >= 400   # every face of the fan got the edge's new vertex


def test_a_face_that_names_a_vertex_twice_is_kept_next_to_a_marked_edge():
    v = np.array([[0.0, 0, 0], [2.0, 0, 0], [1.0, 1.5, 0], [1.0, -1.5, 0]])
    f = np.array([[0, 1, 2], [0, 1, 1], [1, 0, 3], [2, 2, 2], [0, 0, 3]], dtype=np.int64)
    want = check((v, f), max_edge=1.0)
    assert want["report"]["degenerate_kept"] == 3
    for t in ([0, 1, 1], [2, 2, 2], [0, 0, 3]):
        assert (want["faces"] == np.array(t)).all(1).sum() == 1


def test_vertices_that_are_no_numbers_mark_nothing():
    v, f = fo.patch(65, seed=3)
    v = v.copy()
    v[5, 0], v[17, 1], v[30, 2], v[31] = np.nan, np.inf, -np.inf, [np.nan, np.inf, 0.0]
    want = check((v, f), max_edge=0.9)
    assert np.isnan(want["verts"]).any() and want["report"]["converged"]
    check((v, f), min_verts=300)
    nothing = np.full((3, 3), np.nan)
    r = check((nothing, np.array([[0, 1, 2]])), min_verts=10)["report"]
    assert r["stalled"] and not r["converged"] and r["passes"] == 0


def test_a_call_without_any_face_launches_on_nothing_and_stalls():
    empty = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    loose = (np.arange(12.0).reshape(4, 3), np.zeros((0, 3), dtype=np.int64))
    for mesh in (empty, loose):
        r = check(mesh, max_edge=0.5, min_verts=9)["report"]
        assert r["stalled"] and r["passes"] == 0 and r["verts"] == len(mesh[0])
        assert check(mesh, max_edge=0.5)["report"]["converged"]


def test_an_edge_exactly_at_the_limit_stays_and_one_ulp_above_splits():
    L = 1.0 + 2.0 ** -30
    up = np.nextafter(L, 2.0)
    v = np.array([[0.0, 0, 0], [L, 0, 0], [0.5, 0.5, 0], [0.0, 0, 7], [up, 0, 7], [0.5, 0.5, 7]])    # the same x: the differences are exact
    want = check((v, np.array([[0, 1, 2], [3, 4, 5]])), max_edge=L)
    assert fo.sq(v[1], v[0]) == L * L and fo.sq(v[4], v[3]) > L * L
    assert want["report"]["edges_split"] == [1] and want["history"][0][1] == [(3, 4)]


def test_a_budget_that_cuts_through_a_run_of_equal_lengths():
    v, f = fo.box()
    want = check((v, f), min_verts=8 + 6 + 3)
    diagonals = [e for e, l in fo.edge_lengths(v, f).items() if l == 2.0]
    units = sorted(e for e, l in fo.edge_lengths(v, f).items() if l == 1.0)
    assert len(diagonals) == 6 and want["history"][0][1] == sorted(diagonals + units[:3]) and want["report"]["edges_split"] == [9]


def test_a_face_outside_its_mesh_raises():
    v, f = fo.box()
    with pytest.raises(ValueError, match="refine: a face names a vertex outside its mesh"):
        meshprep.refine([v, v], [f, np.array([[0, 1, 8]])], max_edge=0.5)


# ------------------------------------------------------------------------------------------------------------------------- batches
def test_a_batch_equals_its_meshes_alone_bit_for_bit_and_twice():
    meshes = [fo.box(1, 0.13, 2.7), to.torus(6, 5), (fo.disc(9)[0] * 6.0, fo.disc(9)[1]), sized(65), (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))]
    kw = dict(max_edge=0.45, min_verts=400)
    runs = [meshprep.refine([m[0] for m in meshes], [m[1] for m in meshes], return_report=True, **kw) for _ in range(2)]
    passes = [r["passes"] for r in runs[0][1]]
    assert len(set(passes[:4])) == 4                                              # they finish in different passes
    for b, m in enumerate(meshes):
        alone, report = meshprep.refine(m[0], m[1], return_report=True, **kw)
        for run in runs:
            for x, y in zip(alone, run[0][b]):
                assert torch.equal(x.view(torch.int64) if x.is_floating_point() else x, y.view(torch.int64) if y.is_floating_point() else y)
            assert run[1][b] == report
        same(alone, fo.refine(*m, **kw), report)


def test_max_passes_is_a_cap_and_no_error():
    want = check(fo.box(), max_edge=0.3, max_passes=1)
    assert not want["report"]["converged"] and want["report"]["passes"] == 1
    assert check(fo.box(), max_edge=0.3)["report"] == dict(want["report"], passes=3, edges_split=[18, 72, 96], faces_kept=0, faces_split_1=192,
                                                           faces_split_3=60, converged=True, verts=194, faces=384)


# ------------------------------------------------------------------------------------------------------------------------- interpolate
@functools.lru_cache(maxsize=None)
def three_levels():
    r = fo.refine(*fo.box(), max_edge=0.3)
    assert r["report"]["passes"] == 3
    return r["parents"]


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("shape", ((), (1,), (3,), (4,), (67,), (5, 3), (2, 8)))
def test_interpolate_on_three_pass_levels(dtype, shape):
    parents = three_levels()
    x = np.random.default_rng(len(shape) + sum(shape)).standard_normal((8,) + shape).astype(dtype)
    x[3] = np.nan if shape == (3,) else x[3]
    got = meshprep.interpolate(torch.from_numpy(x).cuda(), torch.from_numpy(parents).cuda())
    want = fo.interpolate(x, parents)
    assert got.dtype == torch.from_numpy(x).dtype and tuple(got.shape) == want.shape
    g = got.cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want)) and np.where(np.isnan(g), 0, g).tobytes() == np.where(np.isnan(want), 0, want).tobytes()
    assert np.array_equal(g[:8], x, equal_nan=True)


def test_interpolate_takes_lists_and_refuses_parents_that_are_not_lower():
    parents = three_levels()
    x = np.random.default_rng(0).random((8, 4)).astype(np.float32)
    a, b = meshprep.interpolate([x, x[:, :1]], [parents, parents[:26]])
    assert np.array_equal(a.cpu().numpy(), fo.interpolate(x, parents)) and np.array_equal(b.cpu().numpy(), fo.interpolate(x[:, :1], parents[:26]))
    bad = parents.copy()
    bad[30] = (2, 30)
    with pytest.raises(ValueError, match="interpolate: a parent is not a lower vertex"):
        meshprep.interpolate(x, bad)


# ------------------------------------------------------------------------------------------------------------------------- prepare_mesh
def test_prepare_mesh_gives_every_vertex_of_a_refined_box_a_ball_neighbour():
    v, f = fo.box(1.0, 0.6, 0.8)

    def lonely(d):
        src, dst = d["geo_edge_index"].cpu().numpy()
        has = np.zeros(len(d["verts"]), dtype=bool)
        has[src[src != dst]] = True
        return int((~has).sum())
    coarse = meshprep.prepare_mesh(v, f)
    assert lonely(coarse) == 8 and "parents" not in coarse
    fine = meshprep.prepare_mesh(v, f, refine_max_edge=0.06)
    assert lonely(fine) == 0
    normed = coarse["verts"].cpu().numpy()
    want = fo.refine(normed, f, max_edge=0.06)
    same((fine["verts"], fine["faces"], fine["parents"], fine["face_map"]), want)
    assert torch.equal(fine["vertex_map"].cpu(), torch.arange(8)) and fine["scale"] == coarse["scale"]
    assert fo.longest_edge2(want["verts"], want["faces"]) <= 0.06 * 0.06
