"""GPU: the tolerance weld of ``morig_amd.meshprep.diagnose`` / ``clean`` / ``repair`` / ``prepare_mesh`` (csrc/proxweld.hip) against
tests/proxweld_oracle.py, which is brute force over all pairs of nodes with no grid. Everything is compared with ``==`` / ``torch.equal``
or as bytes (a NaN row is a NaN row on both sides), nothing excused: every field of the report with ``weld_links``, ``near_verts`` and
the bits of ``weld_spread``, and ``clean``'s four outputs. The sizes are those at which a kernel takes another path or a run crosses a
wave (64) or a workgroup (256); the meshes of a test go through the device in ONE batch with per-mesh tolerances.

The issue of this feature also asked to show that ``prepare_mesh`` voxelizes the jittered seam cube to the shell only on the exact path.
It does not: the six loose sheets still cover every surface voxel (a crack of 1e-9 is far below a voxel), so the grid is solid on both
paths -- tests/meshprep_oracle.py gives 4096 of 4096 voxels at dims = 16 for all four of exact / tolerance x clean / repair. What does
differ, and is asserted below: the exact path leaves 24 vertices in 6 components and fans six "holes" (30 vertices, 36 faces), the
tolerance path gives the closed cube of 8 vertices with nothing to fill."""
import functools

import numpy as np
import pytest
import torch

import proxweld_oracle as po
import repair_oracle as ro
import topology_oracle as to
from morig_amd import meshprep

pytestmark = pytest.mark.gpu

NODE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)
CELL_COUNTS = (1, 2, 64, 65, 300)
E3, F3 = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)


def paired_cloud(n, eps, seed):
    """n distinct points: random ones, each followed by a partner at 0.3 to 1.5 tolerances, and random faces over them"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0, 1, ((n + 1) // 2, 3))
    d = rng.standard_normal(base.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    v = np.stack([base, base + d * eps * rng.uniform(0.3, 1.5, (len(base), 1))], 1).reshape(-1, 3)[:n]
    v = v[rng.permutation(n)]
    f = rng.integers(0, n, (n, 3)) if n >= 3 else F3
    return v, f


def one_cell(n, eps, seed):
    """n points within a cube of diagonal below eps: one cell, all linked"""
    v = np.random.default_rng(seed).uniform(0, 0.99 * eps / np.sqrt(3.0), (n, 3)) + 3.0
    return v, (np.arange(3 * (n // 3)).reshape(-1, 3) if n >= 3 else F3)


def damaged():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0.0, 0.0], [1 + 1e-9, 0, 0], [0, 1, 1e-9], [np.nan, 0, 0], [np.inf, 1, 1], [1, 0, 0],
                  [5, 5, 5], [1 - 1e-9, 1e-9, 0], [0, 0, 1], [0, 1e-9, 1], [-np.inf, 0, 0], [1, 0, 0]])
    f = np.array([[0, 1, 2], [3, 4, 5], [0, 8, 11], [3, 10, 12], [6, 7, 9], [2, 5, 9], [0, 3, 9], [14, 2, 11]])
    return v, f


def flat(eps):
    g = np.array([[i, j, 0.0] for i in range(9) for j in range(9)]) * 0.125
    return np.concatenate([g, g + [0.6 * eps, -0.6 * eps, 0.0]]), np.array([[i, i + 1, i + 9] for i in range(70)])


def border_cases():
    out = {}
    for eps in (0.25, 1e-3):                                                      # the tolerance sets the cell
        h = eps * (1.0 + 2.0 ** -20)
        out.update({f"border_{eps}_{frac}": (po.border_pairs(eps, h, frac, 1000.0 * eps), F3, eps) for frac in (0.0, 0.9)})
    for extent in (1000.0, 1e-3):                                                 # the clamp: eps below extent / 2^20
        h = extent * 2.0 ** -20
        out.update({f"clamp_{extent}_{frac}": (po.border_pairs(h / 8.0, h, frac, extent), F3, h / 8.0) for frac in (0.0, 1.0 - 1.0 / 16.0)})
    return out


@functools.lru_cache(maxsize=None)
def cases():
    c = {f"nodes_{n}": (*paired_cloud(n, 1e-4, n), 1e-4) for n in NODE_COUNTS}
    c.update({f"cell_{n}": (*one_cell(n, 1e-3, n), 1e-3) for n in CELL_COUNTS})
    c["chain_1025"] = (*po.chain(1025, 0.9 * 2.0 ** -10), 2.0 ** -10)
    rng = np.random.default_rng(9)
    c["chain_1025_shuffled"] = (po.chain(1025, 0.9 * 2.0 ** -10, axis=2)[0][rng.permutation(1025)], rng.integers(0, 1025, (300, 3)), 2.0 ** -10)
    c["threshold_at"] = (np.array([[0.0, 0, 0], [0.25, 0, 0]]), F3, 0.25)
    c["threshold_above"] = (np.array([[0.0, 0, 0], [0.25 * (1 + 2.0 ** -52), 0, 0]]), F3, 0.25)
    c["threshold_3_4_5"] = (np.array([[0.0, 0, 0], [0.1875, 0.25, 0]]), F3, 0.3125)
    c.update(border_cases())
    c["one_cell_cube"] = (*po.seam_cube(), 2.0)                                   # eps above the extent
    c["flat"] = (*flat(1e-5), 1e-5)
    c["single_point"] = (np.array([[1.0, 2.0, 3.0]]), F3, 0.5)
    c["all_coincident"] = (np.full((130, 3), 0.25), np.random.default_rng(0).integers(0, 130, (70, 3)), 1e-3)
    c["damaged"] = (*damaged(), 1e-8)
    c["seam_cube"] = (*po.seam_cube(), 1e-8)
    c["seam_torus"] = (*po.seam_torus(24, 16), 1e-8)
    c["clusters"] = (*po.clusters(9, 40, 0.5e-4), 1e-4)
    c["empty"] = (E3, F3, 1e-3)
    for eps in (1e-160, 2.0 ** -511):                                             # a subnormal square links nothing; the smallest normal one links
        h = eps * (1.0 + 2.0 ** -20)
        c[f"tiny_line_{eps}"] = (po.subnormal_square(eps), F3, eps)
        c.update({f"tiny_border_{eps}_{frac}": (po.border_pairs(eps, h, frac, 1000.0 * eps), F3, eps) for frac in (0.0, 0.9)})
    return c


@functools.lru_cache(maxsize=None)
def wanted(name):
    """the oracle's answer, computed once and shared"""
    v, f, eps = cases()[name]
    return po.diagnose(v, f, eps), po.clean(v, f, eps)


def same_bits(t, a):
    x = t.cpu().numpy()
    return x.dtype == a.dtype and x.shape == a.shape and x.tobytes() == a.tobytes()


def check(names, out, reports):
    for name, o, r in zip(names, out, reports):
        want_r, want_c = wanted(name)
        for k in to.FIELDS + ("watertight", "rounds") + po.WELD_FIELDS:
            assert r[k] == want_r[k], (name, k, r[k], want_r[k])
        for x, y, k in zip(o, want_c, ("verts", "faces", "vertex_map", "face_map")):
            assert same_bits(x, y), (name, k)


def run(names, **kw):
    cs = cases()
    return meshprep.clean([cs[n][0] for n in names], [cs[n][1] for n in names], weld_tol=[cs[n][2] for n in names], return_report=True, **kw)


def test_every_case_in_one_batch_equals_the_brute_force():
    names = list(cases())
    check(names, *run(names))
    r = dict(zip(names, run(names)[1]))
    assert [r[f"cell_{n}"]["weld_links"] for n in CELL_COUNTS] == [n * (n - 1) // 2 for n in CELL_COUNTS] and r["cell_300"]["weld_links"] == 44850
    assert (r["threshold_at"]["weld_links"], r["threshold_above"]["weld_links"], r["threshold_3_4_5"]["weld_links"]) == (1, 0, 1)
    assert r["chain_1025"]["near_verts"] == 1024 and r["chain_1025"]["weld_spread"] > r["chain_1025"]["weld_tol"]
    assert r["chain_1025_shuffled"]["near_verts"] == 1024 and r["one_cell_cube"]["weld_links"] == 276
    assert r["all_coincident"]["weld_links"] == 0 and r["all_coincident"]["duplicate_verts"] == 129 and r["single_point"]["near_verts"] == 0
    for k in (n for n in names if n.startswith(("border", "clamp"))):
        assert 26 + 1 <= r[k]["weld_links"] <= 3 * 26 + 1                         # every direction links at least once; the top corner links
    assert [r[f"tiny_line_{eps}"]["weld_links"] for eps in (1e-160, 2.0 ** -511)] == [0, 1]
    assert r["tiny_border_1e-160_0.0"]["weld_links"] == r["tiny_border_1e-160_0.9"]["weld_links"] == 0
    s = r["seam_cube"]
    assert (s["components"], s["watertight"], s["euler"], s["duplicate_verts"], s["weld_links"], s["near_verts"]) == (1, True, 2, 16, 24, 16)


@pytest.mark.parametrize("name", ["nodes_1", "nodes_64", "nodes_257", "nodes_1025", "cell_65", "cell_300", "chain_1025", "border_0.25_0.0", "clamp_1000.0_0.0",
                                  "damaged", "flat", "empty", "tiny_line_1e-160", f"tiny_border_{2.0 ** -511}_0.0"])
def test_a_mesh_alone_gives_what_it_gives_in_the_batch(name):
    check([name], *run([name]))                                                   # B = 1: no sort by mesh


def test_keep_rules_and_unreferenced_vertices_on_the_welded_classes():
    names = ["seam_torus", "damaged", "nodes_257", "clusters"]
    cs = cases()
    for keep, drop in (("largest", True), (2, False)):
        out = meshprep.clean([cs[n][0] for n in names], [cs[n][1] for n in names], weld_tol=[cs[n][2] for n in names], keep=keep, drop_unreferenced=drop)
        for n, o in zip(names, out):
            for x, y in zip(o, po.clean(*cs[n], keep, drop)):
                assert same_bits(x, y), (n, keep)


def test_equal_coordinates_in_two_meshes_never_link_and_two_runs_give_the_same_bits():
    names = ["seam_cube", "seam_cube", "empty", "cell_65", "chain_1025_shuffled"]
    first, second = run(names), run(names)
    check(names, *first)
    for a, b in zip(first[0], second[0]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert first[1] == second[1] and first[1][0] == first[1][1] and first[1][0]["weld_links"] == 24
    cs = cases()
    five = ["nodes_65", "empty", "seam_torus", "cell_2", "flat"]                 # per-mesh tolerances, one mesh empty, against the single runs
    batch = run(five)
    for k, n in enumerate(five):
        alone = run([n])
        assert alone[1][0] == batch[1][k] and all(torch.equal(x, y) for x, y in zip(alone[0][0], batch[0][k])), n
    assert [r["weld_tol"] for r in batch[1]] == [cs[n][2] for n in five]


def test_a_tolerance_of_zero_is_the_exact_weld_and_relative_tolerances_scale_with_the_box():
    ms = [to.split_cube(), to.torus(16, 16, perm=np.random.default_rng(3).permutation(256)), damaged(), po.seam_cube(), paired_cloud(257, 1e-4, 5)]
    a = meshprep.clean([m[0] for m in ms], [m[1] for m in ms], weld_tol=0, return_report=True)
    b = meshprep.clean([m[0] for m in ms], [m[1] for m in ms], weld=True, return_report=True)
    for x, y, ra, rb in zip(a[0], b[0], a[1], b[1]):
        assert all(same_bits(p, q.cpu().numpy()) for p, q in zip(x, y))
        assert {k: ra[k] for k in rb} == rb and (ra["weld_links"], ra["near_verts"], ra["weld_spread"], ra["weld_tol"]) == (0, 0, 0.0, 0.0)
    v, f = damaged()                                                              # a NaN and two infinite rows: the box is that of the finite ones
    reps = meshprep.diagnose([v, po.seam_cube()[0] * 8.0, E3], [f, po.seam_cube()[1], F3], weld_tol=[1e-9, 1e-8, 0.5], weld_tol_rel=True)
    for (vv, ff, t), r in zip(((v, f, 1e-9), (po.seam_cube()[0] * 8.0, po.seam_cube()[1], 1e-8), (E3, F3, 0.5)), reps):
        eps = t * po.diagonal(vv)
        want = po.diagnose(vv, ff, eps)
        assert r["weld_tol"] == eps and all(r[k] == want[k] for k in to.FIELDS + ("watertight", "rounds") + po.WELD_FIELDS)
    assert reps[1]["watertight"]


def test_max_links_raises_before_anything_is_emitted():
    v, f, eps = cases()["cell_65"]
    with pytest.raises(ValueError, match="clean: weld_tol 0.001 of mesh 0 is too large for this mesh: more than max_links = 10 links"):
        meshprep.clean([v], [f], weld_tol=eps, max_links=10)
    with pytest.raises(ValueError, match="diagnose: weld_tol 0.001 of mesh 1 is too large"):
        meshprep.diagnose([E3, v], [F3, f], weld_tol=eps, max_links=10)


def test_clean_repair_and_prepare_mesh_close_the_jittered_seam_cube():
    v, f = po.seam_cube()
    (cv, cf, vmap, fmap), = meshprep.clean([v], [f], weld_tol=1e-8)
    assert cv.shape == (8, 3) and cf.shape == (12, 3) and to.diagnose(cv.cpu().numpy(), cf.cpu().numpy(), weld=False)["watertight"]
    out, reports = meshprep.repair([v, v], [f, f], fill_holes="all", weld_tol=[1e-8, 0.0], return_report=True)
    for o, r, eps in zip(out, reports, (1e-8, 0.0)):
        want = ro.repair(po.moved(v, eps)[0], f, fill_holes="all")
        for x, k in zip(o, ("verts", "faces", "vertex_map", "face_map", "flipped")):
            assert same_bits(x, want[k]), (eps, k)
        assert all(r[k] == want["report"][k] for k in meshprep.REPAIR_FIELDS) and r["input"]["weld_tol"] == eps
    assert (reports[0]["filled_loops"], reports[0]["closed_components"], tuple(out[0][0].shape)) == (0, 1, (8, 3))
    assert (reports[1]["filled_loops"], reports[1]["closed_components"], tuple(out[1][0].shape)) == (6, 0, (30, 3))   # six "holes" fanned
    kw = dict(n_samples=64, oversample=2, dims=16, self_loops=False)
    loose, fixed = meshprep.prepare_mesh(v, f, repair=True, **kw), meshprep.prepare_mesh(v, f, repair=True, weld_tol=1e-8, **kw)
    print("voxels set: exact path", int(loose["vox"].data.sum()), "tolerance path", int(fixed["vox"].data.sum()), "of", 16 ** 3)
    assert fixed["vox"].data[8, 8, 8] and fixed["vox"].data.all()                # solid
    assert loose["vox"].data.all()                                               # and so is the exact path: cracks of 1e-9 leak nothing
    assert fixed["verts"].shape == (8, 3) and fixed["faces"].shape == (12, 3) and loose["verts"].shape == (30, 3) and loose["faces"].shape == (36, 3)
    assert fixed["report"]["input"]["watertight"] and fixed["report"]["input"]["weld_links"] == 24 and not loose["report"]["input"]["watertight"]
    assert fixed["tpl_edge_index"].shape[1] == 36 and loose["tpl_edge_index"].shape[1] > 36   # one surface: 18 edges both ways
    with pytest.raises(ValueError, match="prepare_mesh: weld_tol belongs to the clean / repair step"):
        meshprep.prepare_mesh(v, f, weld_tol=1e-8)
