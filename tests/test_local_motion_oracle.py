"""CPU: tests/local_motion_oracle.py against what the reference's own get_gt_rotation_icp recorded (tests/golden/local_motion.npz, made by
tools/make_local_motion_golden.py), and every named case of the generators against what it is named for."""
import numpy as np
import pytest

import local_motion_oracle as lo

GOLDEN = lo.load_golden()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_oracle_patches_equal_the_recorded_ones(name):
    c = GOLDEN[name]
    want = lo.patch_lists(c["verts0"], c["faces"])
    assert len(want["lists"]) == len(c["nnids"]) == len(c["verts0"])
    for a, b in zip(want["lists"], c["nnids"]):
        assert np.array_equal(a, b) and np.all(np.diff(a) > 0)
    v0, faces, vt = lo.golden_cases()[name]                                             # the golden reproduces from its generator
    assert np.array_equal(v0, c["verts0"]) and np.array_equal(faces, c["faces"]) and np.array_equal(vt, c["verts_t"])


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_oracle_fits_agree_with_the_recorded_ones(name):
    c = GOLDEN[name]
    got = lo.local_motion(c["verts0"], c["verts_t"][:, None], c["nnids"])
    want = dict(got, rot6d=c["R_all"][:, None], trans=c["T_all"][:, None])
    assert c["R_all"].shape == (len(c["verts0"]), 6) and c["T_all"].shape == (len(c["verts0"]), 3)
    lo.assert_motion_close(got, want, c["verts0"], c["verts_t"][:, None], c["nnids"], name)
    for v, ids in enumerate(c["nnids"]):                                                # and Horn's route, within K0 itself
        R, gap = lo.fit_horn(c["verts0"][ids], c["verts_t"][ids])
        assert np.abs(np.concatenate([R[:, 0], R[:, 1]]) - c["R_all"][v]).max() * gap <= lo.K0 * lo.EPS
        assert abs(gap - got["gap"][v, 0]) <= 64 * lo.EPS


def test_k0_is_what_the_measurement_gives():
    measured = lo.measure_k0(verbose=False)
    assert measured <= lo.K0 <= 2.0 * measured                                          # covers the measurement and is not inflated


def test_list_unions_equal_breadth_first_depth_four_on_proper_triangles_only():
    for v, f in (lo.grid_mesh(7, 6, 0.01), lo.strip_mesh(12), lo.fan_mesh(9), lo.shuffled(*lo.grid_mesh(6, 6, 0.01, 2), seed=3)):
        lists, isolated = lo.ring_lists(len(v), f)
        assert not isolated.any() and all(np.array_equal(a, b) for a, b in zip(lists, lo.bfs_depth4(len(v), f)))
    lists, _ = lo.ring_lists(2, np.array([[0, 0, 1]]))                                  # a degenerate face alone: the walks of four edges
    assert [r.tolist() for r in lists] == [[0], [1]] and [r.tolist() for r in lo.bfs_depth4(2, np.array([[0, 0, 1]]))] == [[0, 1], [0, 1]]


def test_the_named_cases_are_what_they_are_named_for():
    v, f = lo.strip_mesh(14)
    got = lo.patch_lists(v, f)
    far = 5                                                                             # vertex 2 * 5 is five hops from vertex 0, at 0.025
    assert lo.dist_row(v[0], v[[2 * far]])[0] < 0.03 and 2 * far not in got["lists"][0] and 2 * 4 in got["lists"][0]
    assert (got["rung"] == 0).all()
    for n_near, far_r, rung, size in ((3, (0.045, 0.07), 1, 5), (4, (0.07,), 0, 5), (3, (0.07, 0.07), 2, 4), (2, (0.045, 0.055, 0.07), 2, 5),
                                      (2, (0.045, 0.07, 0.07), 2, 4), (1, (0.045, 0.045, 0.055), 2, 5)):
        v, f = lo.rung_mesh(n_near, far_r)
        got = lo.patch_lists(v, f)
        assert got["rung"][0] == rung and len(got["lists"][0]) == size, (n_near, far_r, got["rung"][0], len(got["lists"][0]))
    v, f = lo.exact_rung_mesh()
    got = lo.patch_lists(v, f)
    assert lo.dist_row(v[0], v[[1]])[0] == lo.RUNGS[2] == 0.0625 and got["rung"][0] == 2 and 1 not in got["lists"][0]
    v, f = lo.fan_mesh(100)
    assert len(lo.patch_lists(v, f)["lists"][0]) == 101
    v, f = lo.isolated_mesh()
    got = lo.patch_lists(v, f)
    assert got["n_isolated"] == 1 and got["lists"][-1].tolist() == [len(v) - 1] and all(len(v) - 1 not in r for r in got["lists"][:-1])


def test_fit_cases():
    rng = np.random.default_rng(0)
    src = rng.normal(size=(12, 3)) * 0.02
    R = lo.rotation([1, 2, 3], np.pi)                                                   # 180 degrees
    got, _, s, d = lo.fit_svd(src, src @ R.T + 0.1)
    assert np.abs(got - R).max() < 1e-13 and d == 1.0
    flat_src = src * [1, 1, 0]
    mirrored = flat_src * [1, -1, 1]                                                    # a mirrored planar patch: the fit is a half turn about x
    got, t, s, d = lo.fit_svd(flat_src, mirrored)
    assert abs(np.linalg.det(got) - 1.0) < 1e-13 and s[2] < 1e-18 and np.abs(got - np.diag([1.0, -1.0, -1.0])).max() < 1e-12
    one = lo.local_motion(src, (src + 0.25)[:, None], [[3]] * len(src))
    assert np.array_equal(one["rot6d"][0, 0], [1, 0, 0, 0, 1, 0]) and np.allclose(one["trans"], 0.25) and (one["gap"] == 0).all()
