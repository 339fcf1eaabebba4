"""CPU: (1) the host logic of morig_amd/playback.py on an emulated op layer (tests/playback_emulate.py through ``runtime._test_ops``): the
ragged tables, the tree-order tables, entries from ``skin_entries_device`` against those from dense ``skins``, the slicing of a batch,
T mismatch and status handling; (2) csrc/pose_core.h as the stand-alone program tools/pose_host_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a program (never loaded into Python), bit for bit against tests/playback_oracle.py on every
fixture."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import playback_emulate as pe
import playback_oracle as po
from morig_amd import playback, runtime, tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META, CASES = po.load_cases()
BY_NAME = {c["name"]: c for c in CASES}
T_BATCH = po.FRAME_TILE + 1


@pytest.fixture()
def ops():
    emu = pe.PlaybackOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def batch_inputs(cases=CASES, T=T_BATCH):
    return [pe.make_rig(c) for c in cases], [c["vtx"] for c in cases], [pe.stretch(c["quats"], T) for c in cases]


# ------------------------------------------------------------------------------------------------------------------------- tables
def test_rig_tables_hold_the_tree_order_and_the_fk_inputs(ops):
    rigs, _, _ = batch_inputs()
    rt = playback.RigTables(rigs, torch.device("cpu"), "test")
    jp = rt.jptr.numpy()
    assert rt.jptr.dtype == rt.parent.dtype == rt.order.dtype == rt.pos_f32.dtype == torch.int32
    assert list(jp) == list(np.concatenate([[0], np.cumsum([c["J"] for c in CASES])]))
    for m, c in enumerate(CASES):
        rows = slice(jp[m], jp[m + 1])
        order = tracking.tree_order(c["hier"], c["root_id"])[0]
        assert np.array_equal(rt.order.numpy()[rows], order) and order[0] == c["root_id"]
        assert np.array_equal(rt.parent.numpy()[rows], c["hier"]) and rt.parent.numpy()[rows][c["root_id"]] == -1
        off = c["offset"].copy()
        off[c["root_id"]] = c["pos"][c["root_id"]]
        assert np.array_equal(rt.offsets.numpy()[rows], off)
        assert np.array_equal(rt.bind.numpy()[rows, :9].reshape(-1, 3, 3), c["bind_G"]) and np.array_equal(rt.bind.numpy()[rows, 9:], c["pos"])
        assert bool(rt.pos_f32[m]) == (c["pos"].dtype == np.float32)
    root = rt.root_positions(None, 3, torch.device("cpu"), "test")
    assert root.shape == (len(CASES), 3, 3) and np.array_equal(root[4, 2].numpy(), CASES[4]["pos"][CASES[4]["root_id"]])


def test_skin_tables_from_dense_skins_and_from_device_entries_agree(ops):
    cases = [BY_NAME["j23"], BY_NAME["noweight"], BY_NAME["posed"]]
    dense = [pe.make_rig(c) for c in cases]
    sparse = []
    for c in cases:
        vptr, ev, ej, w = tracking.skin_entries(c["skins"])
        rig = pe.make_rig(c, tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (vptr, ev.astype(np.int32), ej.astype(np.int32), w)))
        rig.skins = []                                                          # only the entries are left to read
        sparse.append(rig)
    vtx = [c["vtx"] for c in cases]
    a, b = (playback.SkinTables(r, vtx, torch.device("cpu"), "test") for r in (dense, sparse))
    for k in ("vptr", "eptr", "joint", "weight", "vtx"):
        assert torch.equal(getattr(a, k), getattr(b, k)) and getattr(a, k).is_contiguous(), k
    assert a.eptr.dtype == a.joint.dtype == torch.int32 and a.weight.dtype == torch.float64
    ep, vp = a.eptr.numpy(), a.vptr.numpy()
    assert ep[0] == 0 and ep[-1] == a.joint.numel() == sum(np.count_nonzero(c["skins"]) for c in cases)
    assert ep[vp[1] + 3] == ep[vp[1] + 4]                                       # the vertex without weights owns no entry
    q = [pe.stretch(c["quats"], 4) for c in cases]
    for x, y in zip(playback.skin_trajectory(dense, vtx, q), playback.skin_trajectory(sparse, vtx, q)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------------- results
_cache = {}


def batch_run():
    if "b" not in _cache:
        before = len(runtime._test_ops.calls)
        out = playback.replay(*batch_inputs())
        _cache["b"] = (out, runtime._test_ops.calls[before:])
    return _cache["b"]


def test_ragged_batch_over_the_emulated_ops_equals_the_oracle_bit_for_bit(ops):
    out, calls = batch_run()
    assert calls == ["pose_validate", "pose_quats", "pose_fk", "pose_local", "pose_skin"]          # five launches for the whole batch
    for (traj, q), c in zip(out, CASES):
        want = po.replay(c["rig"], c["vtx"], pe.stretch(c["quats"], T_BATCH))
        assert traj.dtype == q.dtype == torch.float64 and tuple(traj.shape) == (c["V"], T_BATCH, 3) and tuple(q.shape) == (c["J"], T_BATCH, 4)
        assert np.array_equal(traj.numpy(), want["traj"]) and np.array_equal(q.numpy(), want["quats"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_a_mesh_alone_at_its_own_length_equals_the_recorded_reference(ops, case):
    q_in = case["quats"].copy()
    (traj, q), = playback.replay([pe.make_rig(case)], [case["vtx"]], [q_in])
    assert np.array_equal(q_in, case["quats"])                                  # the caller's array is not written
    assert np.array_equal(q.numpy(), case["ref_quats"])
    tol = po.bound(case["depth"], case["scale"])
    assert np.abs(traj.numpy() - case["ref_traj"]).max() <= tol
    (G, pos), = playback.pose_rigs([pe.make_rig(case)], [case["ref_quats"]])
    assert G.dtype == torch.float64 and tuple(G.shape) == (case["J"], case["T"], 3, 3) and str(pos.dtype) == "torch." + str(case["pos"].dtype)
    assert np.abs(G.numpy() - case["ref_G"]).max() <= tol and np.abs(pos.numpy().astype(np.float64) - case["ref_pos"]).max() <= tol
    if "aligned_in" in case:
        (traj_a, q_a), = playback.replay([pe.make_rig(case)], [case["vtx"]], [case["quats"]], align_signs=True)
        assert np.array_equal(q_a.numpy(), case["ref_quats_aligned"]) and np.abs(traj_a.numpy() - case["ref_traj_aligned"]).max() <= tol


def test_a_mesh_alone_equals_its_slice_of_the_batch(ops):
    out, _ = batch_run()
    for i in (0, 3, 8):
        (traj, q), = playback.replay(*batch_inputs([CASES[i]]))
        assert torch.equal(traj, out[i][0]) and torch.equal(q, out[i][1])


def test_smooth_quats_options(ops):
    c = BY_NAME["flip"]
    q = torch.from_numpy(c["quats"])
    plain, = playback.smooth_quats([q])
    assert np.array_equal(plain.numpy(), c["ref_quats"]) and plain.data_ptr() != q.data_ptr() and np.array_equal(q.numpy(), c["quats"])
    aligned, = playback.smooth_quats([c["quats"]], align_signs=True)
    assert np.array_equal(aligned.numpy(), c["ref_quats_aligned"])
    same, = playback.smooth_quats([c["quats"]], passes=0)
    assert np.array_equal(same.numpy(), c["quats"])
    for T in (1, 2, 3):
        got, = playback.smooth_quats([c["quats"][:, :T]], passes=5)
        assert np.array_equal(got.numpy()[:, [0, -1]], c["quats"][:, [0, T - 1]]) and (T == 3 or np.array_equal(got.numpy(), c["quats"][:, :T]))
    strided = torch.from_numpy(np.ascontiguousarray(c["quats"].transpose(1, 0, 2))).permute(1, 0, 2)
    assert not strided.is_contiguous() and torch.equal(playback.smooth_quats([strided])[0], plain)
    assert playback.smooth_quats([]) == [] and playback.replay([], [], []) == []


def test_root_pos_replaces_the_root_per_frame_in_the_rigs_type(ops):
    c = BY_NAME["j23"]                                                          # float32 joints
    rp = np.random.default_rng(2).normal(size=(c["T"], 3))
    (G, pos), = playback.pose_rigs([pe.make_rig(c)], [c["quats"]], root_pos=[rp])
    want_G, want_pos = po.fk(c["rig"], po.quat_matrices(c["quats"]), root_pos=rp)
    assert pos.dtype == torch.float32 and np.array_equal(pos.numpy(), want_pos) and np.array_equal(G.numpy(), want_G)
    assert np.array_equal(pos.numpy()[c["root_id"]], rp.astype(np.float32))
    with pytest.raises(ValueError, match=r"root_pos\[0\] is \[T, 3\]"):
        playback.pose_rigs([pe.make_rig(c)], [c["quats"]], root_pos=[rp[:-1]])


# ------------------------------------------------------------------------------------------------------------------------- errors
def test_shape_errors(ops):
    a, b = BY_NAME["j3"], BY_NAME["noweight"]
    rigs, vtx = [pe.make_rig(a), pe.make_rig(b)], [a["vtx"], b["vtx"]]
    with pytest.raises(ValueError, match="a batch has one T"):
        playback.replay(rigs, vtx, [a["quats"], b["quats"]])
    with pytest.raises(ValueError, match="one row per joint"):
        playback.replay(rigs, vtx, [a["quats"], a["quats"]])
    with pytest.raises(ValueError, match="one entry per mesh"):
        playback.replay(rigs, vtx, [a["quats"]])
    with pytest.raises(ValueError, match="skin rows"):
        playback.skin_trajectory([rigs[0]], [a["vtx"][:-1]], [a["quats"]])
    assert ops.calls == []                                                     # refused before any op
    broken = pe.make_rig(a)
    broken.hierarchy = broken.hierarchy.copy()
    broken.hierarchy[np.nonzero(broken.hierarchy >= 0)[0][0]] = 7
    with pytest.raises(ValueError, match="mesh 1: tree_order"):
        playback.pose_rigs([rigs[0], broken], [a["quats"], a["quats"]])


def test_status_names_the_meshes_and_spares_the_others(ops, monkeypatch):
    cases = [BY_NAME["j3"], BY_NAME["noweight"], BY_NAME["flip"]]
    rigs, vtx, quats = batch_inputs(cases, 4)
    clean = playback.replay(rigs, vtx, quats)
    zero = [q.copy() for q in quats]
    zero[1][2, 1] = 0.0
    with pytest.raises(ValueError, match=r"meshes \[1\]: a quaternion has zero or non-finite norm"):
        playback.replay(rigs, vtx, zero, smooth=False)
    vptr, ev, ej, w = tracking.skin_entries(cases[2]["skins"])
    ej = ej.astype(np.int32)
    ej[5] = cases[2]["J"]                                                       # one past the rig
    bad = pe.make_rig(cases[2], tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (vptr, ev.astype(np.int32), ej, w)))
    with pytest.raises(ValueError, match=r"meshes \[2\]: a joint or parent index"):
        playback.replay([rigs[0], rigs[1], bad], vtx, quats)
    monkeypatch.setattr(playback, "_raise_status", lambda *a: None)             # look at what the launches left behind
    got = playback.replay([rigs[0], rigs[1], bad], vtx, zero, smooth=False)
    unsmoothed = playback.replay(rigs, vtx, quats, smooth=False)
    assert torch.equal(got[0][0], unsmoothed[0][0]) and torch.equal(got[0][1], unsmoothed[0][1])
    assert not torch.equal(clean[0][0], unsmoothed[0][0])


def test_trajectory_errors_over_the_emulated_ops(ops):
    rng = np.random.default_rng(4)
    pred = [rng.normal(size=(v, 6, 3)) for v in (33, 1, 70)]
    gt = [p + rng.normal(size=p.shape) * 0.1 for p in pred]
    mask = [rng.uniform(size=p.shape[:2]) for p in pred]
    res = playback.trajectory_errors(pred, [torch.from_numpy(g) for g in gt], mask)
    assert ops.calls == ["pose_traj_errors"]
    for (full, vis), p, g, m in zip(res, pred, gt, mask):
        d = np.sqrt(((p - g) ** 2).sum(2))
        assert full.shape == vis.shape == (6,) and np.allclose(full.numpy(), d.mean(0), rtol=1e-13, atol=0)
        want_full, want_vis = tracking.flow_errors(p, np.concatenate([g[:, :1], g], 1), np.concatenate([m[:, :1], m], 1))
        assert abs(full.numpy().mean() - want_full) <= 1e-13 * want_full
        seen = m > 0.5
        with np.errstate(all="ignore"):
            per_frame = (d * seen).sum(0) / seen.sum(0)
        assert np.allclose(vis.numpy(), per_frame, rtol=1e-13, atol=0, equal_nan=True)
    with pytest.raises(ValueError, match="one T per batch"):
        playback.trajectory_errors([pred[0], pred[1][:, :5]], [gt[0], gt[1][:, :5]], [mask[0], mask[1][:, :5]])


# ------------------------------------------------------------------------------------------------------------ the host program
def _write_case(f, c, quats, passes, align):
    order = tracking.tree_order(c["hier"], c["root_id"])[0]
    ev, ej, w = po.entries(c["skins"])
    eptr = np.concatenate([[0], np.cumsum(np.bincount(ev, minlength=c["V"]))]).astype(np.int32)
    off = c["offset"].copy()
    off[c["root_id"]] = c["pos"][c["root_id"]]
    T = quats.shape[1]
    root_pos = np.broadcast_to(c["pos"][c["root_id"]].astype(np.float64), (T, 3))
    bind = np.concatenate([c["bind_G"].reshape(-1, 9), c["pos"].astype(np.float64)], 1)
    f.write(struct.pack("7i", c["J"], c["V"], T, len(ej), int(c["pos"].dtype == np.float32), passes, int(align)))
    for a, dt in ((quats, np.float64), (c["hier"], np.int32), (order, np.int32), (off, np.float64), (root_pos, np.float64), (bind, np.float64),
                  (c["vtx"], np.float64), (eptr, np.int32), (ej, np.int32), (w, np.float64)):
        f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    return len(ej)


def test_pose_core_under_the_sanitizers_equals_the_oracle_bit_for_bit(tmp_path):
    exe = str(tmp_path / "pose_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "pose_host_check.cpp"), "-o", exe], check=True)
    runs = [(c, c["quats"], 2, False) for c in CASES] + [(BY_NAME["flip"], BY_NAME["flip"]["quats"], 2, True)]
    zero = BY_NAME["j3"]["quats"].copy()
    zero[1, 1] = 0.0
    runs.append((BY_NAME["j3"], zero, 0, False))                                # a zero quaternion: the status, no trap
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(runs)))
        n_entries = [_write_case(f, c, q, passes, align) for c, q, passes, align in runs]
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    raw, at = open(dst, "rb").read(), 0

    def take(shape):
        nonlocal at
        n = int(np.prod(shape))
        a = np.frombuffer(raw, dtype=np.float64, count=n, offset=at).reshape(shape)
        at += 8 * n
        return a

    for (c, q_in, passes, align), E in zip(runs, n_entries):
        status, = struct.unpack_from("i", raw, at)
        at += 4
        J, V, T = c["J"], c["V"], q_in.shape[1]
        q, xf, local, traj = take((J, T, 4)), take((J, 12, T)), take((E, 3)), take((V, T, 3))
        if q_in is zero:
            assert status == 1
            continue
        want = po.replay(c["rig"], c["vtx"], q_in, smooth_passes=passes, align=align)
        assert status == 0 and np.array_equal(q, want["quats"]), c["name"]
        assert np.array_equal(xf[:, :9].transpose(0, 2, 1).reshape(J, T, 3, 3), want["G"]), c["name"]
        assert np.array_equal(xf[:, 9:].transpose(0, 2, 1), want["pos"].astype(np.float64)), c["name"]
        assert np.array_equal(local, want["local"]) and np.array_equal(traj, want["traj"]), c["name"]
    assert at == len(raw)
