"""GPU: morig_amd/playback.py over csrc/playback.hip against tests/playback_oracle.py (bit for bit) and against the results recorded from
the reference's smooth_quats and Rig.FK (within the rounding bound). Every fixture case runs alone at its recorded clip length, and all of
them run as ONE ragged batch at a common length (the fixture's tracks repeated to T = 65, one past the skinning kernel's frame tile); both
are computed once and shared by the tests."""
import numpy as np
import pytest
import torch

import playback_emulate as pe
import playback_oracle as po
from morig_amd import playback, tracking

pytestmark = pytest.mark.gpu

META, CASES = po.load_cases()
BY_NAME = {c["name"]: c for c in CASES}
T_BATCH = po.FRAME_TILE + 1
DEV = "cuda"
_cache = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def batch_inputs(cases=CASES, T=T_BATCH):
    return [pe.make_rig(c) for c in cases], [dev(c["vtx"]) for c in cases], [dev(pe.stretch(c["quats"], T)) for c in cases]


def alone():
    """every case at its own T: (traj, quats, G, pos) as numpy, and the oracle's dict"""
    if "alone" not in _cache:
        out = []
        for c in CASES:
            (traj, q), = playback.replay([pe.make_rig(c)], [dev(c["vtx"])], [dev(c["quats"])])
            (G, pos), = playback.pose_rigs([pe.make_rig(c)], [q])
            out.append((traj.cpu().numpy(), q.cpu().numpy(), G.cpu().numpy(), pos.cpu().numpy(), po.replay(c["rig"], c["vtx"], c["quats"])))
        _cache["alone"] = out
    return _cache["alone"]


def batch():
    if "batch" not in _cache:
        _cache["batch"] = playback.replay(*batch_inputs())
        _cache["batch_oracle"] = [po.replay(c["rig"], c["vtx"], pe.stretch(c["quats"], T_BATCH)) for c in CASES]
    return _cache["batch"], _cache["batch_oracle"]


# ------------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_each_case_equals_the_oracle_bit_for_bit_and_the_reference_within_the_bound(i):
    c = CASES[i]
    traj, q, G, pos, want = alone()[i]
    assert np.array_equal(q, want["quats"]) and np.array_equal(q, c["ref_quats"])
    assert np.array_equal(G, want["G"]) and pos.dtype == c["pos"].dtype and np.array_equal(pos, want["pos"])
    assert traj.shape == (c["V"], c["T"], 3) and np.array_equal(traj, want["traj"])
    tol = po.bound(c["depth"], c["scale"])
    devs = (np.abs(traj - c["ref_traj"]).max(), np.abs(G - c["ref_G"]).max(), np.abs(pos.astype(np.float64) - c["ref_pos"]).max())
    print(f"{c['name']}: device vs reference traj {devs[0]:.2e} G {devs[1]:.2e} pos {devs[2]:.2e}, bound {tol:.2e}")
    assert max(devs) <= tol


def test_ragged_batch_equals_the_oracle_bit_for_bit():
    got, want = batch()
    for (traj, q), w, c in zip(got, want, CASES):
        assert traj.is_cuda and traj.dtype == q.dtype == torch.float64 and tuple(traj.shape) == (c["V"], T_BATCH, 3)
        assert np.array_equal(q.cpu().numpy(), w["quats"]) and np.array_equal(traj.cpu().numpy(), w["traj"]), c["name"]
    assert torch.all(got[8][0][3] == 0.0)                                       # the vertex without weights


def test_two_runs_and_a_mesh_alone_give_the_bits_of_the_batch():
    got, _ = batch()
    again = playback.replay(*batch_inputs())
    for (a, b), (c, d) in zip(got, again):
        assert torch.equal(a, c) and torch.equal(b, d)
    for i in (0, 4, 7, 9):
        (traj, q), = playback.replay(*batch_inputs([CASES[i]]))
        assert torch.equal(traj, got[i][0]) and torch.equal(q, got[i][1])


def test_aligned_flip_case_equals_the_reference():
    c = BY_NAME["flip"]
    (traj, q), = playback.replay([pe.make_rig(c)], [dev(c["vtx"])], [dev(c["quats"])], align_signs=True)
    want = po.replay(c["rig"], c["vtx"], c["quats"], align=True)
    assert np.array_equal(q.cpu().numpy(), c["ref_quats_aligned"]) and np.array_equal(traj.cpu().numpy(), want["traj"])
    assert np.abs(traj.cpu().numpy() - c["ref_traj_aligned"]).max() <= po.bound(c["depth"], c["scale"])


# ------------------------------------------------------------------------------------------------------------------------- properties
def test_no_passes_and_short_clips_leave_the_end_frames():
    c = BY_NAME["j23"]
    q = dev(c["quats"])
    same, = playback.smooth_quats([q], passes=0)
    assert torch.equal(same, q) and same.data_ptr() != q.data_ptr()
    for T in (1, 2, 3):
        cut = dev(c["quats"][:, :T])
        got, = playback.smooth_quats([cut], passes=4)
        assert torch.equal(got[:, 0], cut[:, 0]) and torch.equal(got[:, -1], cut[:, -1])
        assert np.array_equal(got.cpu().numpy(), po.smooth(c["quats"][:, :T], 4)) and (T == 3 or torch.equal(got, cut))
        (traj, q2), = playback.replay([pe.make_rig(c)], [dev(c["vtx"])], [cut], passes=4)
        assert np.array_equal(traj.cpu().numpy(), po.replay(c["rig"], c["vtx"], c["quats"][:, :T], smooth_passes=4)["traj"])
    assert torch.equal(q, dev(c["quats"]))                                      # the caller's tensor is not written


def test_sign_alignment_changes_no_rotation_of_the_unsmoothed_replay():
    c = BY_NAME["flip"]
    rig, vtx, q = [pe.make_rig(c)], [dev(c["vtx"])], [dev(c["quats"])]
    aligned = playback.smooth_quats(q, passes=0, align_signs=True)
    assert np.array_equal(aligned[0].cpu().numpy(), c["aligned_in"]) and not torch.equal(aligned[0], q[0])
    (G0, p0), = playback.pose_rigs(rig, q)
    (G1, p1), = playback.pose_rigs(rig, aligned)
    assert torch.equal(G0, G1) and torch.equal(p0, p1)
    (t0, _), = playback.replay(rig, vtx, q, smooth=False)
    (t1, q1), = playback.replay(rig, vtx, q, smooth=False, align_signs=True)
    assert torch.equal(t0, t1) and torch.equal(q1, aligned[0])


def test_strided_and_host_inputs_give_the_bits_of_contiguous_ones():
    got, _ = batch()
    rigs, vtx, quats = batch_inputs()
    vtx_s = [torch.cat([v, v], 1).reshape(-1, 2, 3)[:, 0] for v in vtx]
    quats_s = [q.permute(1, 0, 2).contiguous().permute(1, 0, 2) for q in quats]
    assert not vtx_s[3].is_contiguous() and not quats_s[3].is_contiguous()
    host = [q.cpu().numpy() if i % 2 else q for i, q in enumerate(quats_s)]
    for (a, b), (c, d) in zip(got, playback.replay(rigs, vtx_s, host)):
        assert torch.equal(a, c) and torch.equal(b, d)


def test_device_entries_are_used_in_place_of_dense_skins():
    c = BY_NAME["j48"]
    vptr, ev, ej, w = tracking.skin_entries(c["skins"])
    rig = pe.make_rig(c, (dev(vptr), dev(ev.astype(np.int32)), dev(ej.astype(np.int32)), dev(w)))
    rig.skins = []
    (traj, _), = playback.replay([rig], [dev(c["vtx"])], [dev(c["quats"])])
    assert np.array_equal(traj.cpu().numpy(), alone()[4][0])


def test_root_pos_and_a_rig_of_the_largest_supported_size():
    from morig_amd.skeleton import MAX_JOINTS
    J, V, T = MAX_JOINTS, 100, 3                                                # MORIG_PRIM_MAX_JOINTS: no LDS-sized limit applies
    rng = np.random.default_rng(11)
    hier = np.array([-1] + [int(rng.integers(max(0, i - 6), i)) for i in range(1, J)])
    pos = rng.uniform(-0.5, 0.5, (J, 3)).astype(np.float32)
    skins = np.zeros((V, J))
    for v in range(V):
        js = rng.choice(J, 4, replace=False)
        skins[v, js] = rng.uniform(0.1, 1, 4)
    from morig_amd.formats import Rig
    rig = Rig.from_arrays(pos, hier, 0, skins=skins)
    case = dict(pos=rig.pos, hierarchy=rig.hierarchy, root_id=0, offset=rig.offset, global_transforms=rig.global_transforms, skins=skins)
    quats, vtx, rp = rng.normal(size=(J, T, 4)), rng.uniform(-1, 1, (V, 3)), rng.normal(size=(T, 3))
    (traj, q), = playback.replay([rig], [vtx], [quats], root_pos=[rp])
    want = po.replay(case, vtx, quats, root_pos=rp)
    assert np.array_equal(q.cpu().numpy(), want["quats"]) and np.array_equal(traj.cpu().numpy(), want["traj"])
    (G, p), = playback.pose_rigs([rig], [quats], root_pos=[rp])
    assert p.dtype == torch.float32 and np.array_equal(p.cpu().numpy()[0], rp.astype(np.float32))
    assert np.array_equal(G.cpu().numpy(), po.fk(case, po.quat_matrices(quats), root_pos=rp)[0])


# ------------------------------------------------------------------------------------------------------------------------- status paths
def test_a_bad_index_or_a_zero_quaternion_raises_and_spares_the_other_meshes(monkeypatch):
    cases = [BY_NAME["j3"], BY_NAME["noweight"], BY_NAME["flip"]]
    rigs, vtx, quats = batch_inputs(cases, 4)
    clean = playback.replay(rigs, vtx, quats, smooth=False)
    zero = [q.clone() for q in quats]
    zero[1][2, 1] = 0.0
    with pytest.raises(ValueError, match=r"meshes \[1\]: a quaternion has zero or non-finite norm"):
        playback.replay(rigs, vtx, zero, smooth=False)
    nan = [q.clone() for q in quats]
    nan[0][0, 3, 2] = float("nan")
    with pytest.raises(ValueError, match=r"meshes \[0\]: a quaternion"):
        playback.pose_rigs(rigs, nan)
    vptr, ev, ej, w = tracking.skin_entries(cases[2]["skins"])
    ej = ej.astype(np.int32)
    ej[5] = cases[2]["J"]                                                       # one past the rig: a status, never followed
    bad = pe.make_rig(cases[2], (dev(vptr), dev(ev.astype(np.int32)), dev(ej), dev(w)))
    with pytest.raises(ValueError, match=r"meshes \[2\]: a joint or parent index"):
        playback.skin_trajectory([rigs[0], rigs[1], bad], vtx, quats)
    monkeypatch.setattr(playback, "_raise_status", lambda *a: None)             # what the launches left for the other meshes
    got = playback.replay([rigs[0], rigs[1], bad], vtx, zero, smooth=False)
    assert torch.equal(got[0][0], clean[0][0]) and torch.equal(got[0][1], clean[0][1])


def test_validate_flags_parents_and_orders_outside_the_rig():
    from morig_amd.runtime import get_ops
    ops = get_ops()
    jptr = torch.tensor([0, 3, 5, 8], dtype=torch.int32, device=DEV)
    parent = torch.tensor([-1, 0, 1, -1, 2, -1, 0, 1], dtype=torch.int32, device=DEV)        # mesh 1: parent 2 of 2 joints
    order = torch.tensor([0, 1, 2, 0, 1, 0, 1, 3], dtype=torch.int32, device=DEV)            # mesh 2: order 3 of 3 joints
    status = torch.zeros(3, dtype=torch.int32, device=DEV)
    ops.pose_validate(jptr, parent, order, None, None, None, status)
    assert status.tolist() == [0, ops.POSE_BAD_INDEX, ops.POSE_BAD_INDEX]


# ------------------------------------------------------------------------------------------------------------------------- errors
def test_trajectory_errors_against_flow_errors_and_the_oracle():
    rng = np.random.default_rng(8)
    sizes, T = (257, 1, 70, 1030), 66
    pred = [rng.normal(size=(v, T, 3)) for v in sizes]
    gt = [p + rng.normal(size=p.shape) * 0.1 for p in pred]
    mask = [rng.uniform(size=p.shape[:2]) for p in pred]
    mask[2][:, 5] = 0.0                                                         # a frame that sees nothing
    res = playback.trajectory_errors([dev(p) for p in pred], gt, [dev(m) for m in mask])
    for (full, vis), p, g, m in zip(res, pred, gt, mask):
        assert full.is_cuda and full.dtype == torch.float64 and full.shape == vis.shape == (T,)
        want_full, want_vis = po.trajectory_errors(p, g, m)
        assert np.array_equal(full.cpu().numpy(), want_full) and np.array_equal(vis.cpu().numpy(), want_vis, equal_nan=True)
        n = p.shape[0]
        for t in range(0, T, 13):                                               # flow_errors drops frame 0: give it one to drop
            f, v = tracking.flow_errors(p[:, t:t + 1], np.concatenate([g[:, :1], g[:, t:t + 1]], 1), np.concatenate([m[:, :1], m[:, t:t + 1]], 1))
            assert abs(full[t].item() - f) <= n * 2.0 ** -53 * f
            assert (np.isnan(v) and np.isnan(vis[t].item())) or abs(vis[t].item() - v) <= n * 2.0 ** -53 * v
    assert np.isnan(res[2][1][5].item())


def test_output_offsets_past_2_to_the_31():
    """V T 3 > 2^31 doubles: one joint, one weight per vertex, the vertices repeating with period 1024, so that row v must equal row
    v % 1024 -- also in the rows whose element offsets no longer fit 32 bits."""
    T, period = 64, 1024
    V = (2 ** 31 // (3 * T) // period + 2) * period
    assert V * T * 3 > 2 ** 31 + period * T * 3
    from morig_amd.formats import Rig
    rig = Rig.from_arrays(np.array([[0.1, 0.2, 0.3]]), [-1], 0)
    one = torch.ones(V, dtype=torch.float64, device=DEV)
    rig.skin_entries_device = (torch.arange(V + 1, dtype=torch.int32, device=DEV), torch.arange(V, dtype=torch.int32, device=DEV),
                               torch.zeros(V, dtype=torch.int32, device=DEV), one)
    rng = np.random.default_rng(5)
    vtx = dev(rng.uniform(-1, 1, (period, 3))).repeat(V // period, 1)
    quats = dev(rng.normal(size=(1, T, 4)))
    (traj, _), = playback.replay([rig], [vtx], [quats])
    head = traj[:period]
    want = po.replay(dict(pos=rig.pos, hierarchy=[-1], root_id=0, offset=rig.offset, global_transforms=rig.global_transforms,
                          skins=np.ones((period, 1))), vtx[:period].cpu().numpy(), quats.cpu().numpy())["traj"]
    assert np.array_equal(head.cpu().numpy(), want)
    first_past = 2 ** 31 // (3 * T) // period
    for k in (first_past - 1, first_past, first_past + 1, V // period - 1):
        assert torch.equal(traj[k * period:(k + 1) * period], head), k
