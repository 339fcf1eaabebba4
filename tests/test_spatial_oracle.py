"""CPU: the numpy oracle of the mesh BVH (tests/spatial_oracle.py) against itself on the case tables of tests/spatial_cases.py -- its
tree walk must return what its brute force returns on EVERY query of every case, bit for bit (face ids, and NaN against NaN), so that
the GPU test, which compares the device with the brute force, leaves nothing out either; the tree itself; and the amount of pruning on
the structured case, which is where the caps of tests/test_gpu_spatial.py come from."""
import numpy as np
import pytest

import spatial_cases as sc
import spatial_oracle as so
from spatial_cases import POINT_CAP, POINT_SHARE, RAY_CAP, RAY_SHARE


def rays_of(case, b):
    rs = slice(case["ray_ptr"][b], case["ray_ptr"][b + 1])
    return case["origins"][rs], case["dirs"][rs]


@pytest.mark.parametrize("case", sc.all_cases(), ids=lambda c: c["name"])
def test_the_walk_equals_brute_force_on_every_query(case):
    """nothing is excluded: the compared share is 1 by construction (every query of every mesh is compared)"""
    for b, (v, f) in enumerate(case["meshes"]):
        tree = so.build(v, f)
        o, d = rays_of(case, b)
        for orientation in ((0, 1, -1) if case["exact"] or len(o) <= 8 else (0,)):
            got, want = so.cast(tree, o, d, orientation), so.brute_cast(o, d, v, f, orientation)
            assert all(so.same(got[k], want[k]) for k in ("t", "face", "point")) and got["bad"] == want["bad"], (case["name"], b, orientation)
        got, want = so.closest(tree, case["points"][b]), so.brute_closest(case["points"][b], v, f)
        assert all(so.same(got[k], want[k]) for k in ("face", "bary", "distance")), (case["name"], b)
        assert got["bad"] == want["bad"] and got["no_faces"] == want["no_faces"]
        a, e, skip, t_max = sc.segments_of(case, b)
        for kw in (dict(), dict(skip_vertex=skip), dict(skip_vertex=skip, t_max=t_max)):
            assert so.same(so.blocked(tree, a, e, **kw)["blocked"], so.brute_blocked(a, e, v, f, **kw)["blocked"]), (case["name"], b, list(kw))


def test_the_exact_cases_hold_the_ties_they_are_there_for():
    cases = {c["name"]: c for c in sc.exact_cases()}
    v, f = cases["plate_twice"]["meshes"][0]
    o, d = rays_of(cases["plate_twice"], 0)
    hit = so.brute_cast(o, d, v, f)
    assert (hit["face"] >= 0).sum() > 200 and np.all(hit["face"][hit["face"] >= 0] < len(f) // 2)      # the twin never wins
    near = so.brute_closest(cases["plate_twice"]["points"][0], v, f)
    assert (near["distance"] == 0.0).sum() > 200 and np.all(near["face"] < len(f) // 2)
    v, f = cases["same_centroid"]["meshes"][0]
    assert len(np.unique(so.morton_codes(v, f))) == 1 and np.array_equal(so.build(v, f)["order"], np.arange(len(f)))
    v, f = cases["plate_twice"]["meshes"][0]
    assert np.ptp(v[:, 2]) == 0.0                                                       # an axis without extent
    v, f = cases["single_point"]["meshes"][0]
    assert np.all(so.morton_codes(v, f) == 0)                                           # no extent at all


def test_the_segment_cases_hold_what_they_are_there_for():
    case = {c["name"]: c for c in sc.exact_cases()}["plate_twice"]
    v, f = case["meshes"][0]
    a, e, skip, t_max = sc.segments_of(case, 0)
    plain = so.brute_blocked(a, e, v, f)["blocked"]
    o, d = rays_of(case, 0)
    t = so.brute_cast(o, d, v, f)["t"]
    with np.errstate(all="ignore"):
        ts = t / (2.0 ** (np.arange(len(a)) % 4 - 1))                                  # the hit in the segment's own parameter: exact
    assert np.array_equal(plain, (ts < 1.0).astype(np.uint8)) and (ts == 1.0).sum() > 20       # the end point itself does not block
    skipped = so.brute_blocked(a, e, v, f, skip_vertex=skip)["blocked"]
    assert np.all(skipped <= plain) and (skipped < plain).sum() > 10                    # the only blocking faces name the vertex
    limited = so.brute_blocked(a, e, v, f, t_max=t_max)["blocked"]
    at = (np.arange(len(a)) % 5 == 0) & (t < np.inf)
    assert not limited[at].any() and plain[at].any()                                    # a hit exactly at t_max does not block


@pytest.mark.parametrize("nf,levels", [(0, []), (1, [1]), (64, [1]), (65, [2, 1]), (4096, [64, 1]), (4097, [65, 2, 1]), (64 ** 3 + 1, [4097, 65, 2, 1]),
                                       (64 ** 4, [64 ** 3, 4096, 64, 1])])
def test_level_counts(nf, levels):
    assert so.level_counts(nf) == levels


def test_the_tree_is_exact_and_ordered():
    v, f = sc.surface_mesh(4097, seed=1)
    tree = so.build(v, f)
    codes = so.morton_codes(v, tree["faces"])[tree["order"]]
    assert np.all(np.diff(codes) >= 0) and np.array_equal(np.sort(tree["order"]), np.arange(len(f)))
    same_code = np.diff(codes) == 0
    assert np.all(np.diff(tree["order"])[same_code] > 0)                               # stable: equal codes in ascending face order
    tri = v[f]
    assert so.same(tree["levels"][-1][0], np.concatenate([tri.min((0, 1)), tri.max((0, 1))]))
    assert [len(lv) for lv in tree["levels"]] == [65, 2, 1]
    one = so.build(v, f[tree["order"][:64]])
    assert so.same(one["levels"][0][0], tree["levels"][0][0])                           # a node is a function of its faces alone


def test_pruning_on_the_structured_case():
    """The torus of 4 096 faces: 168 bone rays, 256 points near the surface. Measured with this oracle: rays 0.1076 of Q x F, points
    0.0687; the caps are these x 1.5 -- 0.162 and 0.103 -- and hold for the device too (the same traversal rule)."""
    case = sc.structured_case()
    v, f = case["meshes"][0]
    tree = so.build(v, f)
    o, d = rays_of(case, 0)
    rays, pts = so.cast(tree, o, d), so.closest(tree, case["points"][0])
    ray_share = rays["visits"].sum() / (len(o) * len(f))
    point_share = pts["visits"].sum() / (len(case["points"][0]) * len(f))
    print(f"ray share {ray_share:.4f} (cap {RAY_CAP}), point share {point_share:.4f} (cap {POINT_CAP})")
    assert abs(ray_share - RAY_SHARE) < 5e-4 and abs(point_share - POINT_SHARE) < 5e-4  # the docstring's figures are the measured ones
    assert ray_share < RAY_CAP and point_share < POINT_CAP
    assert (rays["face"] >= 0).mean() > 0.9
