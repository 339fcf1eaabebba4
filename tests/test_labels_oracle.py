"""CPU: tests/labels_oracle.py itself -- known answers (a torus with a joint chain on its core circle, an axis-aligned box with a centre
joint, the on-grid rays), the percentile formula against np.percentile, and the condition of the GPU tests shown satisfiable: on the
generated scenes the oracle alone leaves out at most a thousandth of a case's rays and vertices. Also the C ABI of the new entry points:
declared, exported, refusing bad sizes without a device."""
import numpy as np
import pytest

import labels_oracle as lo
from morig_amd import abi, labels, native


@pytest.mark.parametrize("n_side", lo.GENERATED_SIDES)
def test_torus_feature_size_is_the_tube_radius_and_the_margins_hold(n_side):
    v, f, pos, hier = lo.generated_scene(n_side)
    want = lo.generated_reference(n_side)
    R, V = len(want["t"]), len(v)
    assert R == 168 and (want["face"] >= 0).all() and (want["n_hit"] == 14).all()
    fs = want["featuresize"]
    share = want["attn"].mean()
    soft_rays = int((want["ray_margin"] < lo.MARGIN).sum() + ((want["keep_margin"] < lo.MARGIN) & (want["ray_margin"] >= lo.MARGIN)).sum())
    soft_verts = int((want["radius_margin"] < lo.RADIUS_MARGIN).sum())
    print(f"torus {n_side}: featuresize {fs.min():.4f} .. {fs.max():.4f}, kept {int(want['kept'].sum())} of {R}, labelled {100 * share:.1f} % of {V}, "
          f"smallest margins: ray {want['ray_margin'].min():.2e}, keep {want['keep_margin'].min():.2e}, radius {want['radius_margin'].min():.2e}")
    assert np.all(np.abs(fs - 0.12) < 0.012)                                            # the tube radius, a facetted and noisy surface
    assert 0.02 < share < 0.3 and want["attn"].dtype == np.float32 and set(np.unique(want["attn"])) == {0.0, 1.0}
    assert soft_rays <= 0.001 * R and soft_verts <= 0.001 * V                           # the condition of tests/test_gpu_labels.py
    # every hit lies on the surface: within the noise of the tube around the core circle
    p = want["point"]
    tube = np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 2] ** 2) - 0.35) ** 2 + p[:, 1] ** 2)
    assert np.all(np.abs(tube - 0.12) < 0.02)
    assert np.allclose(np.linalg.norm(want["dirs"], axis=1), 1.0, atol=1e-15)
    o = want["origins"]
    assert np.allclose(np.linalg.norm(p - o, axis=1), want["t"], atol=1e-14)            # d is unit up to rounding: t is the distance


def test_percentile_formula_equals_numpy():
    worst = 0.0
    for n_side in lo.GENERATED_SIDES:
        want = lo.generated_reference(n_side)
        for j in range(12):
            tj = want["t"][14 * j:14 * j + 14]
            worst = max(worst, abs(want["p20"][j] - np.percentile(tj, 20)))
    for n in (1, 2, 3, 4, 5, 6, 7, 11, 14, 16, 64, 65, 1024):
        t = lo.hit_set(n, 3)
        hits = np.sort(t[t < np.inf])
        worst = max(worst, abs(lo.p20_of(hits) - np.percentile(hits, 20)))
    print(f"p20 against np.percentile: largest difference {worst:.2e}")
    assert worst <= 1e-15


def test_box_with_a_centre_joint_has_exact_distances():
    for hy, fs_want, kept_want in ((0.2, 0.1625, 4), (0.375, 0.125, 2)):
        v, f = lo.box_mesh(0.5, hy, 0.125)
        got = lo.labels(v, f, [[0, 0, 0], [0.25, 0, 0]], [-1, 0], n_rays=4)
        assert list(got["counts"]) == [4, 4] and list(got["n_hit"]) == [4, 4]         # the leaf casts about its parent's axis
        want_t = np.array([0.125, hy, 0.125, hy] * 2)                                   # u = +z, w = -y
        assert np.all(np.abs(got["t"] - want_t) <= 1e-15)
        assert list(got["n_kept"]) == [kept_want] * 2 and np.all(np.abs(got["featuresize"] - fs_want) <= 1e-15)
        assert np.all(np.abs(got["p20"] - 0.125) <= 1e-15)
    flipped = lo.labels(v, f[:, ::-1], [[0, 0, 0], [0.25, 0, 0]], [-1, 0], n_rays=4, orientation=1)
    plain = lo.labels(v, f, [[0, 0, 0], [0.25, 0, 0]], [-1, 0], n_rays=4, orientation=1)
    assert {int(flipped["n_hit"].sum()), int(plain["n_hit"].sum())} == {0, 8}           # one winding faces the rays, the other does not


def test_on_grid_rays_have_the_stated_answers():
    v, f, o, d, names = lo.on_grid_scene()
    res = {k: lo.cast(o, d, v, f, k) for k in (0, 1, -1)}
    at = {n: i for i, n in enumerate(names)}
    face, t = res[0]["face"], res[0]["t"]
    for n, (fw, tw) in dict(inside=(0, 2.0), shared_edge=(0, 2.0), corner=(0, 2.0), far_corner=(0, 0.75), outer_edge=(0, 2.0), from_above=(0, 1.0),
                            two_plates=(3, 2.0), two_plates_down=(2, 2.0), zero_area=(5, 2.0), nan_vertex=(7, 2.0), twins=(8, 2.0)).items():
        assert (face[at[n]], t[at[n]]) == (fw, tw), n
    for n in ("outside", "coplanar", "behind", "on_the_face", "nan_ray", "zero_dir", "sideways"):
        assert face[at[n]] == -1 and t[at[n]] == np.inf and np.isnan(res[0]["point"][at[n]]).all(), n
    assert np.array_equal(res[0]["point"][at["far_corner"]], [1.0, 1.0, 2.0])
    # +z rays meet the +z normals: orientation +1 keeps them; the nearest hit of the wrong orientation is a miss, the ray does not continue
    assert res[1]["face"][at["inside"]] == 0 and res[-1]["face"][at["inside"]] == -1
    assert res[1]["face"][at["from_above"]] == -1 and res[-1]["face"][at["from_above"]] == 0
    assert res[-1]["face"][at["two_plates"]] == -1 and res[1]["face"][at["two_plates"]] == 3
    assert res[-1]["face"][at["two_plates_down"]] == -1 and res[1]["face"][at["two_plates_down"]] == 2


def test_the_c_abi_declares_types_and_refuses_without_a_device():
    names = ["morig_ray_cast", "morig_ray_select", "morig_ray_attention"]
    assert set(names) <= set(native.EXPORTS) and len(abi.STRUCTS) == 8                 # plain parameters: no new argument struct
    lib = native.load_library()
    K = abi.CONSTANTS
    assert K["MORIG_RAY_MAX_PER_JOINT"] == labels.MAX_RAYS_PER_JOINT == 1024 and K["MORIG_RAY_STATS"] == 4
    assert lib.morig_ray_select(None, None, 3, 1025, 2.0, 0.0, None, None, None) == K["MORIG_E_UNSUPPORTED"]    # before anything is launched
    assert lib.morig_ray_select(None, None, -1, 4, 2.0, 0.0, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_ray_select(None, None, 3, 4, 2.0, 0.0, None, None, None) == K["MORIG_E_INVALID"]           # null pointers
    assert lib.morig_ray_select(None, None, 0, 0, 2.0, 0.0, None, None, None) == K["MORIG_OK"]
    assert lib.morig_ray_cast(None, None, None, 4, None, None, None, None, 1, 0, None, None, None, None, None) == K["MORIG_E_INVALID"]   # no status word
    assert lib.morig_ray_cast(None, None, None, -1, None, None, None, None, 1, 0, None, None, None, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_ray_attention(None, None, None, 1, -1, None, None, None, 0.02, None, None) == K["MORIG_E_INVALID"]
    assert lib.morig_ray_attention(None, None, None, 1, 0, None, None, None, 0.02, None, None) == K["MORIG_OK"]  # no vertices
    assert lib.morig_ray_attention(None, None, None, 1, 2, None, None, None, 0.02, None, None) == K["MORIG_E_INVALID"]
    prof = [lib.morig_prof_name(k) for k in range(K["MORIG_PROF_KINDS"])]
    assert b"ray_cast" in prof and b"ray_select" in prof and b"ray_attention" in prof
