"""Host side of morig_amd/tracking.py without a GPU: formats.Rig's pose state and the rig update chain bit for bit against the reference's
recorded rigs, the selection on the explicit ``corrmat`` path with the exact pair lists, the packing of a batch for morig_ik_solve, and
ik_drag's glue end to end with the float64 oracle standing in for the device solver."""
import numpy as np
import pytest

import tracking_oracle as tk
from morig_amd import formats, tracking
from test_tracking_oracle import DRAG, DRAG_META, SOLVE, SOLVE_META, solve_problem


def drag_rig(name):
    J, V = len(DRAG[f"{name}_pos"]), len(DRAG[f"{name}_vtx_src"])
    skins = np.zeros((V, J))
    skins[DRAG[f"{name}_skin_v"], DRAG[f"{name}_skin_j"]] = DRAG[f"{name}_skin_w"]
    return formats.Rig.from_arrays(DRAG[f"{name}_pos"], DRAG[f"{name}_parent"], DRAG_META["params"][name]["root"], skins=skins)


def test_rig_pose_state_after_load():
    rig = drag_rig("small")
    J = len(rig.pos)
    assert rig.local_frames.shape == (J, 3, 3) and rig.local_frames.dtype == np.float64
    assert np.array_equal(rig.local_frames, np.repeat(np.eye(3)[None], J, 0)) and np.array_equal(rig.global_transforms, rig.local_frames)
    before = rig.pos.copy()
    rig.fk()                                             # identity frames: the positions the loader already rebuilt
    assert np.array_equal(rig.pos, before) and np.array_equal(rig.global_transforms, np.repeat(np.eye(3)[None], J, 0))
    h = rig.global_transforms_homogeneous
    assert h.shape == (J, 4, 4) and h.dtype == np.float64 and np.array_equal(h[:, :3, 3], rig.pos) and np.array_equal(h[:, 3], [[0, 0, 0, 1]] * J)


@pytest.mark.parametrize("name", DRAG_META["cases"])
def test_rig_update_chain_bit_for_bit(name):
    """pos <- jpos, local_frames <- locals (float32), fk(): float32 global transforms and positions, float64 offsets whose root row takes the
    float32 root position, products rounded on store -- both updates of ik_drag, every array equal to the reference's"""
    rig = drag_rig(name)
    for stage in (1, 2):
        rig = tracking.update_rig(rig, DRAG[f"{name}_solve{stage}_jpos"], DRAG[f"{name}_solve{stage}_locals"])
        for k in ("pos", "local_frames", "global_transforms", "offset"):
            got, want = getattr(rig, k), DRAG[f"{name}_rig{stage}_{k}"]
            assert got.dtype == want.dtype and np.array_equal(got, want), (stage, k)
    assert rig.pos.dtype == np.float32 and rig.offset.dtype == np.float64
    assert tk.quat_distance(tracking.quat_from_matrix(rig.local_frames), DRAG[f"{name}_quats"]) <= 1e-12


@pytest.mark.parametrize("name", DRAG_META["cases"])
def test_selection_from_an_explicit_corrmat(name):
    corr = np.matmul(DRAG[f"{name}_vtx_feature"], DRAG[f"{name}_pts_feature"].T)
    winner, best = tracking.winners_from_corrmat(corr)
    w0, b0, _ = tk.select_pairs(corr.max(1).astype(np.float64), corr.argmax(1), corr.shape[1])
    assert np.array_equal(winner, w0) and np.array_equal(best, b0)
    pairs1, pairs2 = tracking.keep_pairs(winner, best, DRAG[f"{name}_stage1_vtx"], DRAG[f"{name}_pts"])
    assert np.array_equal(pairs1, DRAG[f"{name}_pairs_similarity"]) and np.array_equal(pairs2, DRAG[f"{name}_pairs"])


def test_selection_rule_ties_and_sign():
    """the first vertex wins an exact tie, a non-positive maximum never wins, a point nobody chose has no winner"""
    corr = np.array([[0.9, 0.1, 0.0], [0.9, 0.2, 0.0], [-0.5, -0.2, -0.9], [0.3, 0.95, 0.0]], dtype=np.float32)
    winner, best = tracking.winners_from_corrmat(corr)
    assert winner.tolist() == [0, 3, -1] and best.tolist() == [np.float32(0.9), np.float32(0.95), 0.0]


def test_tree_order_and_packing():
    order, level_ptr, lo, hi = tracking.tree_order([2, 2, -1, 0, 0, 1], 2)
    assert order.tolist() == [2, 0, 1, 3, 4, 5] and level_ptr.tolist() == [0, 1, 3, 6]
    assert [order[lo[j]:hi[j]].tolist() for j in range(6)] == [[3, 4], [5], [0, 1], [], [], []]
    for name in ("chain", "star_root3", "tree_w_invis", "one_joint"):
        prob = solve_problem(SOLVE, SOLVE_META, name)
        mine, theirs = tracking.tree_order(prob["parent"], prob["root"]), tk.bfs(prob["parent"], prob["root"])
        assert all(np.array_equal(a, b) for a, b in zip(mine, theirs))
    with pytest.raises(ValueError):
        tracking.tree_order([1, 0, -1], 2)               # a cycle beside the root
    probs = []
    for name in ("chain", "two_joints_one_vertex"):
        par = SOLVE_META["params"][name]
        p = solve_problem(SOLVE, SOLVE_META, name)
        probs.append(tracking.make_problem(p["locals_in"], p["offsets"], p["parent"], p["root"], p["vptr"], p["ent_j"], p["ent_w"], p["ent_x"],
                                           p["constraints"], p["vismask"], par["iter_time"], par["lr"], par["w_invis"], par["thrd"]))
    t, n, max_j, max_v, max_iter, joint_ptr, vert_ptr = tracking.pack_problems(probs, "cpu")
    assert (n, max_j, max_v, max_iter) == (2, 8, 65, 200) and joint_ptr == [0, 8, 10] and vert_ptr == [0, 65, 66]
    E = [len(p["ent_j"]) for p in probs]
    assert t["vptr"].tolist()[-2:] == [E[0], E[0] + E[1]] and t["jptr"][8].item() == E[0] and t["jptr"][-1].item() == sum(E)
    # the joint-major copy holds the same entries
    ev = np.repeat(np.arange(65), np.diff(probs[0]["vptr"]))
    a = sorted(zip(probs[0]["ent_j"].tolist(), ev.tolist(), probs[0]["ent_w"].tolist()))
    jj = np.repeat(np.arange(8), np.diff(t["jptr"][:9].numpy()))
    b = sorted(zip(jj.tolist(), t["jent_v"][:E[0]].tolist(), t["jent_xw"].view(-1, 4)[:E[0], 3].tolist()))
    assert a == b
    assert t["bias1"][0].item() == 1 - 0.9 and t["bias2_sqrt"][1].item() == (1 - 0.999 ** 2) ** 0.5
    with pytest.raises(ValueError):
        tracking.make_problem(p["locals_in"], p["offsets"], p["parent"], p["root"], p["vptr"], p["ent_j"] + 2, p["ent_w"], p["ent_x"],
                              p["constraints"], p["vismask"])


def oracle_solver(problems, with_grad=False, device=None):
    out = []
    for p in problems:
        r = tk.solve(p, p["iter_time"], p["lr"], p["w_invis"], p["thrd"])
        out.append({k: r[k].astype(np.float32) for k in ("angles", "trans", "locals", "globals", "jpos")})
    return out


@pytest.mark.parametrize("name", ["small"])
def test_ik_drag_glue_with_the_oracle_as_solver(name, monkeypatch):
    """local vertices, both rig updates, selection, the second problem's rows and the final skinning around a float64 solver: the
    reference's pair lists exactly, its vertices and quaternions to the solver's accuracy"""
    monkeypatch.setattr(tracking, "ik_solve", oracle_solver)
    corr = np.matmul(DRAG[f"{name}_vtx_feature"], DRAG[f"{name}_pts_feature"].T)
    details = []
    vtx, rigs, quats = tracking.ik_drag([DRAG[f"{name}_vtx_src"]], [DRAG[f"{name}_vtx_dst"]], [DRAG[f"{name}_pts"]], [drag_rig(name)],
                                        vismask=[DRAG[f"{name}_vismask"]], corrmat=[corr], details=details)
    d = details[0]
    assert np.array_equal(d["pairs_similarity"], DRAG[f"{name}_pairs_similarity"]) and np.array_equal(d["pairs"], DRAG[f"{name}_pairs"])
    assert np.abs(d["stage1_vtx"] - DRAG[f"{name}_stage1_vtx"]).max() <= 2e-6
    assert np.abs(vtx[0] - DRAG[f"{name}_vtx"]).max() <= 2e-6
    assert np.abs(rigs[0].local_frames - DRAG[f"{name}_rig2_local_frames"]).max() <= 2e-6
    assert tk.quat_distance(quats[0], DRAG[f"{name}_quats"]) <= 2e-6
    # without features and corrmat only the first solve runs
    vtx1, rig1, _ = tracking.ik_drag([DRAG[f"{name}_vtx_src"]], [DRAG[f"{name}_vtx_dst"]], [DRAG[f"{name}_pts"]], [drag_rig(name)],
                                     vismask=[DRAG[f"{name}_vismask"]])
    assert np.abs(vtx1[0] - DRAG[f"{name}_stage1_vtx"]).max() <= 2e-6


def test_flow_errors():
    rng = np.random.default_rng(1)
    pred, gt, vis = rng.normal(size=(30, 4, 3)), rng.normal(size=(30, 5, 3)), rng.uniform(size=(30, 5))
    full, seen = tracking.flow_errors(pred, gt, vis)
    d = np.linalg.norm(pred - gt[:, 1:], axis=2)
    assert full == pytest.approx(d.mean(), rel=1e-14) and seen == pytest.approx(d[vis[:, 1:] > 0.5].mean(), rel=1e-13)
