"""CPU: tests/playback_oracle.py, the numpy restatement of csrc/playback.hip in the kernels' order, held to the results recorded from the
reference's own smooth_quats and Rig.FK (tests/golden/playback_cases.npz, tools/make_playback_golden.py): smoothed quaternions bit for
bit, trajectories and forward kinematics within the first-order rounding bound, the fixture conditions, the error paths."""
import numpy as np
import pytest

import playback_oracle as po

META, CASES = po.load_cases()
BY_NAME = {c["name"]: c for c in CASES}


def test_fixture_covers_the_stated_cases():
    shapes = {(c["J"], c["V"], c["T"]) for c in CASES}
    assert {(1, 5, 1), (2, 63, 2), (3, 65, 3), (23, 257, 7), (48, 130, 33)} <= shapes
    assert {c["T"] for c in CASES} >= {po.FRAME_TILE, po.FRAME_TILE + 1}
    assert {str(c["pos"].dtype) for c in CASES} == {"float32", "float64"}
    assert all(c["root_id"] != 0 for c in CASES if c["J"] > 1) and all(c["hier"][c["root_id"]] == -1 for c in CASES)
    eye = np.eye(3)
    assert all(np.array_equal(c["bind_G"], np.broadcast_to(eye, c["bind_G"].shape)) == (c["name"] != "posed") for c in CASES)
    assert np.abs(BY_NAME["posed"]["bind_G"] - eye).max() > 0.1
    assert np.all(BY_NAME["noweight"]["skins"][3] == 0.0) and all(np.all(c["skins"].sum(1) > 0) for c in CASES if c["name"] != "noweight")
    flip = BY_NAME["flip"]
    changed = np.nonzero(np.any(flip["aligned_in"] != flip["quats"], axis=2))
    assert set(changed[0]) == {2} and set(changed[1]) == {3, 4} and np.array_equal(flip["aligned_in"][2, 3], -flip["quats"][2, 3])
    steps = [np.arccos(np.clip(np.abs(po.dot4(c["quats"][:, 1:], c["quats"][:, :-1])), 0, 1)) * 2 for c in CASES if c["T"] > 1]
    assert 0.05 < np.median(np.concatenate([s.reshape(-1) for s in steps])) < 0.3           # about 0.15 rad per frame


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_smoothed_quaternions_equal_the_reference_bit_for_bit(case):
    before = case["quats"].copy()
    got = po.smooth(case["quats"])
    assert np.array_equal(got, case["ref_quats"]) and np.array_equal(case["quats"], before)          # and the input is not written
    assert np.array_equal(got[:, [0, -1]], before[:, [0, -1]])
    if case["T"] < 3:
        assert np.array_equal(got, before)
    if "aligned_in" in case:
        assert np.array_equal(po.align_signs(case["quats"]), case["aligned_in"])
        assert np.array_equal(po.smooth(case["quats"], align=True), case["ref_quats_aligned"])
        assert not np.array_equal(case["ref_quats_aligned"], case["ref_quats"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_trajectory_and_fk_within_the_rounding_bound_of_the_reference(case):
    for suffix, q_in, align in [("", case["quats"], False)] + ([("_aligned", case["quats"], True)] if "aligned_in" in case else []):
        mine = po.replay(case["rig"], case["vtx"], q_in, align=align)
        traj, G, P = case["ref_traj" + suffix], case["ref_G" + suffix], case["ref_pos" + suffix]
        scale = max(np.abs(traj).max(), np.abs(P).max())
        tol = po.bound(case["depth"], scale)
        devs = (np.abs(mine["traj"] - traj).max(), np.abs(mine["G"] - G).max(), np.abs(mine["pos"].astype(np.float64) - P.astype(np.float64)).max())
        print(f"{case['name']}{suffix}: traj {devs[0]:.2e} G {devs[1]:.2e} pos {devs[2]:.2e}, bound {tol:.2e} (depth {case['depth']}, scale {scale:.3g}); "
              f"recorded {case['deviation' + suffix]:.2e}")
        assert po.level_order(case["hier"], case["root_id"])[1] == case["depth"]
        assert max(devs) <= tol and mine["traj"].shape == (case["V"], case["T"], 3)
        assert mine["pos"].dtype == P.dtype == case["pos"].dtype
        if P.dtype == np.float32:
            assert np.array_equal(mine["pos"], P)                               # the float32 stores agree exactly (midpoint condition)


def test_float32_positions_stay_clear_of_rounding_midpoints():
    seen = 0
    for c in CASES:
        if c["pos"].dtype != np.float32 or c["J"] < 2:
            continue
        exact = []
        po.fk(c["rig"], po.quat_matrices(po.smooth(c["quats"])), unrounded=exact)
        margin = po.midpoint_margin(np.concatenate([e.reshape(-1) for e in exact]))
        assert margin > META["margin"] == 2.0 ** -40, (c["name"], margin)
        seen += 1
    assert seen >= 4
    assert po.midpoint_margin([1.0 + 2.0 ** -24]) == 0.0 and po.midpoint_margin([1.0]) > 1e-8


def test_a_vertex_without_weights_gives_zeros_and_a_posed_bind_is_inverted():
    c = BY_NAME["noweight"]
    assert np.all(po.replay(c["rig"], c["vtx"], c["quats"])["traj"][3] == 0.0)
    c = BY_NAME["posed"]
    inv, t = po.inverse_transforms(c["bind_G"], c["pos"].astype(np.float64))
    h = np.zeros((c["J"], 4, 4))
    h[:, :3, :3], h[:, :3, 3], h[:, 3, 3] = c["bind_G"], c["pos"], 1.0
    want = np.linalg.inv(h)
    assert np.abs(inv - want[:, :3, :3]).max() < 1e-14 and np.abs(t - want[:, :3, 3]).max() < 1e-14


def test_sign_alignment_changes_no_rotation():
    c = BY_NAME["flip"]
    assert np.array_equal(po.quat_matrices(c["aligned_in"]), po.quat_matrices(c["quats"]))
    q = np.array([[[0.0, 0, 0, 1], [1.0, 0, 0, 0], [-1.0, 0, 0, 0], [0, 0, 0, -1.0]]])       # dot products 0, -1, 0
    assert np.array_equal(po.align_signs(q)[0], [[0, 0, 0, 1], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, -1]])    # an exact 0 keeps the sign


def test_zero_and_non_finite_norms_raise():
    c = BY_NAME["j3"]
    for bad in (0.0, np.nan, np.inf):
        q = c["quats"].copy()
        q[1, 2] = bad
        with pytest.raises(ValueError, match="zero or non-finite"):
            po.replay(c["rig"], c["vtx"], q, smooth_passes=0)


def test_trajectory_errors_against_the_plain_means():
    rng = np.random.default_rng(3)
    pred, gt = rng.normal(size=(37, 5, 3)), rng.normal(size=(37, 5, 3))
    mask = rng.uniform(size=(37, 5))
    mask[:, 4] = 0.0                                                            # a frame that sees nothing: 0 / 0
    full, vis = po.trajectory_errors(pred, gt, mask)
    d = np.sqrt(((pred - gt) ** 2).sum(2))
    seen = mask > 0.5
    assert np.abs(full - d.mean(0)).max() <= 37 * 2.0 ** -53 * d.mean(0).max()
    assert np.abs(vis[:4] - (d * seen).sum(0)[:4] / seen.sum(0)[:4]).max() <= 37 * 2.0 ** -53 * d.max() and np.isnan(vis[4])
