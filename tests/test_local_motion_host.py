"""CPU: the host logic of morig_amd/local_motion.py on an emulated op layer (tests/local_motion_emulate.py through
``runtime._test_ops``): ragged batches, an empty mesh, an empty batch, every refusal, ``Patches.from_lists``, ``gt_rotation_icp`` -- and
csrc/localfit_core.h as the stand-alone program tools/localfit_host_check.cpp, built with the address and undefined-behaviour
sanitizers and run as a program."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import local_motion_emulate as le
import local_motion_oracle as lo
from morig_amd import local_motion as lm
from morig_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops():
    emu = le.LocalOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def same(a, b):
    a, b = (x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def batch():
    none = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    return [lo.grid_mesh(6, 5, 0.012, seed=1), lo.isolated_mesh(), none, lo.rung_mesh(3, (0.045, 0.07)), lo.exact_rung_mesh(),
            (np.zeros((1, 3)), np.zeros((0, 3), dtype=np.int64))]


def test_patches_of_a_ragged_batch_equal_the_oracle(ops):
    meshes = batch()
    pat = lm.patches([m[0] for m in meshes], [m[1] for m in meshes])
    assert ops.calls == ["transfer_keys", "local_patches", "local_patches"]
    assert pat.n == len(meshes) and pat.nv.tolist() == [len(m[0]) for m in meshes] and pat.n_isolated == 2
    assert pat.ptr.dtype == pat.ids.dtype == pat.rung.dtype == torch.int32
    split = pat.split()
    for b, (v, f) in enumerate(meshes):
        want = lo.patch_lists(v, f)
        assert len(split[b]) == len(v) and all(same(a, w) for a, w in zip(split[b], want["lists"]))
        assert same(pat.rung[pat.vptr_host[b]:pat.vptr_host[b + 1]], want["rung"])
    alone = lm.patches([meshes[3][0]], [meshes[3][1]])
    assert all(same(a, b) for a, b in zip(alone.split()[0], split[3]))
    ops.calls.clear()
    for empty in (lm.patches([], []), lm.patches([meshes[2][0]], [meshes[2][1]])):      # an empty batch, a batch of an empty mesh
        assert empty.ptr.tolist() == [0] and empty.ids.numel() == 0 and ops.calls == []
    assert lm.patches([], []).split() == [] and lm.patches([meshes[2][0]], [meshes[2][1]]).split() == [[]]
    assert lm.RUNGS == lo.RUNGS and lm.RUNGS[2] == 0.0625 and lm.RUNGS[2] > 0.06


def test_patch_refusals(ops):
    v, f = lo.grid_mesh(4, 4, 0.01, seed=2)
    with pytest.raises(ValueError, match="one faces array per mesh"):
        lm.patches([v, v], [f])
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        lm.patches([v[:, :2]], [f])
    with pytest.raises(ValueError, match="at most 32768 per mesh"):
        lm.patches([np.zeros((lm.MAX_VERTS + 1, 3))], [f])
    assert ops.calls == []                                                              # refused before any op
    for bad in (f + 1, np.concatenate([f, [[0, -1, 2]]])):
        with pytest.raises(ValueError, match="outside its mesh"):
            lm.patches([v, v], [f, bad])
    for bad in (np.nan, np.inf, -np.inf):
        moved = v.copy()
        moved[5, 1] = bad
        with pytest.raises(ValueError, match="no finite number"):
            lm.patches([v, moved], [f, f])


def test_local_rigid_motion_of_a_ragged_batch_equals_the_oracle(ops):
    meshes = [m for m in batch() if len(m[0]) != 1]
    verts, faces = [m[0] for m in meshes], [m[1] for m in meshes]
    pat = lm.patches(verts, faces)
    trajs = [lo.bend_clip(v, 3, 40 + b) if len(v) else np.zeros((0, 3, 3)) for b, v in enumerate(verts)]
    ops.calls.clear()
    out = lm.local_rigid_motion(verts, trajs, pat)
    assert ops.calls == ["local_fit"] and out.n_empty == 0 and tuple(out.rot6d.shape) == (sum(len(v) for v in verts), 3, 6)
    split = pat.split()
    for b, (rot6d, trans, gap, residual) in enumerate(out.split()):
        want = lo.local_motion(verts[b], trajs[b], split[b])
        assert same(rot6d, want["rot6d"]) and same(trans, want["trans"]) and same(gap, want["gap"]) and same(residual, want["residual"])
    R = lm.rotation_matrices(out.rot6d)
    assert tuple(R.shape) == tuple(out.rot6d.shape[:2]) + (3, 3) and same(R[..., 0], out.rot6d[..., :3]) and same(R[..., 1], out.rot6d[..., 3:])
    assert np.abs((R @ R.transpose(-1, -2)).numpy() - np.eye(3)).max() < 1e-13 and np.abs(torch.linalg.det(R).numpy() - 1).max() < 1e-13
    f32 = lm.local_rigid_motion(verts, [torch.as_tensor(t, dtype=torch.float32) for t in trajs], pat)
    want = lo.local_motion(verts[0], trajs[0].astype(np.float32), split[0])
    assert same(f32.split()[0][0], want["rot6d"])
    ops.calls.clear()
    none = lm.local_rigid_motion([], [], lm.patches([], []))
    no_frames = lm.local_rigid_motion(verts[:1], [np.zeros((len(verts[0]), 0, 3))], lm.patches(verts[:1], faces[:1]))
    assert tuple(none.rot6d.shape) == (0, 0, 6) and tuple(no_frames.trans.shape) == (len(verts[0]), 0, 3) and "local_fit" not in ops.calls
    with pytest.raises(ValueError, match="one number of frames"):
        lm.local_rigid_motion(verts[:2], [trajs[0], trajs[1][:, :2]], lm.patches(verts[:2], faces[:2]))
    with pytest.raises(ValueError, match="other vertex counts"):
        lm.local_rigid_motion(verts[1:3], trajs[1:3], lm.patches(verts[:2], faces[:2]))
    with pytest.raises(ValueError, match="one rest pose"):
        lm.local_rigid_motion(verts[:2], trajs[:1], lm.patches(verts[:2], faces[:2]))
    with pytest.raises(ValueError, match=r"\[V, T, 3\]"):
        lm.local_rigid_motion(verts[:1], [trajs[0][:, 0]], lm.patches(verts[:1], faces[:1]))


def test_from_lists_and_the_drop_in(ops):
    v, f = lo.grid_mesh(5, 4, 0.012, seed=3)
    vt = lo.bend_clip(v, 1, 9)[:, 0]
    R_all, T_all, nnids = lm.gt_rotation_icp(v, f, vt)
    want_lists = lo.patch_lists(v, f)["lists"]
    want = lo.local_motion(v, vt[:, None], want_lists)
    assert all(same(a, b) for a, b in zip(nnids, want_lists)) and same(R_all, want["rot6d"][:, 0]) and same(T_all, want["trans"][:, 0])
    again = lm.gt_rotation_icp(v, f, vt, nnids)                                         # the lists handed back, as the reference's callers do
    assert same(again[0], R_all) and same(again[1], T_all) and again[2] is nnids
    own = [list(r) for r in want_lists]
    own[2], own[7] = [], [7]                                                            # an empty row, a patch of one point
    pat = lm.Patches.from_lists([own])
    assert pat.n_empty == 1 and (pat.rung == -1).all() and [r.tolist() for r in pat.split()[0]] == [list(map(int, r)) for r in own]
    out = lm.local_rigid_motion([v], [vt[:, None]], pat)
    assert out.n_empty == 1 and torch.isnan(out.rot6d[2]).all() and torch.isnan(out.trans[2]).all() and torch.isnan(out.gap[2]).all()
    assert out.rot6d[7, 0].tolist() == [1, 0, 0, 0, 1, 0] and same(out.trans[7, 0], vt[7] - v[7]) and out.gap[7, 0] == 0
    for bad in ([[len(v)]] + own[1:], [[-1]] + own[1:], [[0.5]] + own[1:]):
        with pytest.raises(ValueError, match="from_lists"):
            lm.Patches.from_lists([bad])


def test_localfit_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "localfit_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "localfit_host_check.cpp"), "-o", exe], check=True)
    ladders = np.array([[a, b, c] for a in (0, 4, 5, 9) for b in (4, 5) for c in (0, 4, 5, 70)], dtype=np.int32)
    pairs = np.array([[0, 0, 0, 0.0625, 0, 0], [0, 0, 0, 0.03, 0.04, 0], [1e-200, 0, -0.0, 0, 0, 0.0], [0.1, 0.2, 0.3, 0.1, 0.2, 0.3]])
    sets = []
    for name, (v0, faces, vt) in lo.golden_cases().items():
        sets.append((name, v0, vt[:, None], lo.patch_lists(v0, faces)["lists"]))
    v, f = lo.fan_mesh(100)
    lists = [list(r) for r in lo.patch_lists(v, f)["lists"]]
    lists[1], lists[2], lists[3], lists[4] = [], [2], [2, 50], [1, 40, 80]              # empty, 1, 2 and 3 points; the hub has 101
    sets.append(("fan", v, lo.bend_clip(v, 5, 3), lists))
    sets.append(("nothing", np.zeros((0, 3)), np.zeros((0, 2, 3)), []))
    for name, v0, traj, lists in sets:
        ptr, ids = lo.flat([np.asarray(r, dtype=np.int64) for r in lists])
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("=iiiii", len(v0), traj.shape[1], len(ids), len(ladders), len(pairs)))
            for a in (ptr, ids, v0, traj, ladders, pairs):
                fh.write(np.ascontiguousarray(a).tobytes())
        done = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", (name, done.returncode, done.stderr[-2000:])
        raw = open(dst, "rb").read()
        n = len(v0) * traj.shape[1]
        res = np.frombuffer(raw[:88 * n], dtype=np.float64).reshape(len(v0), traj.shape[1], 11)
        rungs = np.frombuffer(raw[88 * n:88 * n + 4 * len(ladders)], dtype=np.int32)
        dists = np.frombuffer(raw[88 * n + 4 * len(ladders):], dtype=np.float64)
        assert rungs.tolist() == [0 if a >= 5 else (1 if b >= 5 else 2) for a, b, c in ladders]
        assert same(dists, np.array([lo.dist_row(p[:3], p[None, 3:])[0] for p in pairs])) and dists[0] == lo.RUNGS[2] and dists[2] == 0.0
        got = dict(rot6d=res[..., :6].copy(), trans=res[..., 6:9].copy(), gap=res[..., 9].copy(), residual=res[..., 10].copy())
        if name == "fan":                                                               # rank <= 1 patches: properties only
            for v_, size in ((2, 1), (3, 2)):
                assert (got["gap"][v_] <= 1e-12).all()
            assert np.array_equal(got["rot6d"][2, 0], [1, 0, 0, 0, 1, 0]) and np.array_equal(got["trans"][2], traj[2] - v0[2])
            lists[2], lists[3] = [], []
            for k in got:
                got[k][2:4] = np.nan
        lo.assert_motion_close(got, lo.local_motion(v0, traj, lists), v0, traj, lists, name)
