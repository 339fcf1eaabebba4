"""CPU: the host logic of morig_amd/labels.py on an emulated op layer (tests/labels_emulate.py through ``runtime._test_ops``): the ray plan
against a loop over the joints, ragged batches, the refusals, the files and their round trip through ``formats.load_rig_sample``, the
feature sizes going through ``metrics.evaluate_rigs`` (tests/metrics_emulate.py), and csrc/boneray_core.h as the stand-alone program
tools/boneray_host_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import labels_emulate as le
import labels_oracle as lo
from morig_amd import formats, labels, runtime, skinning
from morig_amd.formats import Rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops():
    emu = le.LabelOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def same(a, b):
    a, b = (x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def tree_rig(seed=0):
    """root 0 with children 1, 2, 5; 1 -> 3; 3 -> 4 coincident with 3 (no axis: 3 casts about its parent's); 2 a leaf; 5 -> 6, 7"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.3, 0.3, size=(8, 3))
    pos[4] = pos[3]
    return lo.PlainRig(pos, [-1, 0, 0, 1, 3, 0, 5, 5])


def plan_by_loop(rigs, n_rays):
    parts = [lo.bone_rays(r.pos, r.hierarchy, n_rays) for r in rigs]
    cat = lambda k, shape, dt: np.concatenate([p[k] for p in parts]) if parts else np.zeros(shape, dtype=dt)
    ptr = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    return (cat(0, (0, 3), np.float64), cat(1, (0, 3), np.float64), ptr([len(p[0]) for p in parts]), ptr(cat(3, (0,), np.int64)), cat(2, (0,), np.int64))


# ------------------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("n_rays", [1, 2, 5, 14, 64])
def test_bone_rays_equal_a_loop_over_the_joints(n_rays):
    lone, far_leaf = lo.PlainRig([[0.1, 0.2, 0.3]], [-1]), lo.PlainRig([[0, 0, 0], [0, 0, 0], [0, 0.5, 0]], [-1, 0, 1])
    rigs = [tree_rig(1), lone, lo.PlainRig(*lo.torus_chain()), far_leaf, tree_rig(2)]
    got = labels.bone_rays(rigs, n_rays)
    for g, w in zip(got, plan_by_loop(rigs, n_rays)):
        assert same(g, w)
    per_joint = np.diff(got.joint_ptr)
    assert list(per_joint[:8] // n_rays) == [3, 1, 1, 1, 0, 2, 1, 1]                    # multi-child, leaf, coincident child, its child
    assert per_joint[8] == 0                                                            # a root alone: no axis, no rays
    assert list(per_joint[21:24] // n_rays) == [0, 1, 1]                                # the coincident pair: only the far bone counts
    assert np.allclose(np.linalg.norm(got.dirs, axis=1), 1.0, atol=1e-15)
    axis = np.repeat(np.arange(len(got.dirs) // n_rays), n_rays)
    assert got.joint_ptr[-1] == got.ray_ptr[-1] == len(got.origins) and len(np.unique(axis)) == per_joint.sum() // n_rays


def test_bone_rays_refusals_and_empty_input():
    for bad in (0, 65, -3):
        with pytest.raises(ValueError, match="n_rays"):
            labels.bone_rays([tree_rig()], bad)
    star = lo.PlainRig(np.concatenate([[[0, 0, 0]], np.random.default_rng(0).uniform(0.1, 1, (17, 3))]), [-1] + [0] * 17)
    assert np.diff(labels.bone_rays([star], 60).joint_ptr).max() == 1020
    with pytest.raises(ValueError, match="1088 rays"):
        labels.bone_rays([star], 64)
    with pytest.raises(ValueError, match="hierarchy"):
        labels.bone_rays([lo.PlainRig([[0, 0, 0]], [3])], 4)
    empty = labels.bone_rays([], 14)
    assert empty.origins.shape == (0, 3) and list(empty.ray_ptr) == [0] and list(empty.joint_ptr) == [0]


# ------------------------------------------------------------------------------------------------------------------------- the stages
def test_labels_of_a_ragged_batch_equal_the_oracle(ops):
    v16, f16, pos, hier = lo.generated_scene(16)
    bv, bf = lo.box_mesh(0.5, 0.2, 0.125)
    none_v, none_f = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    meshes = [(v16, f16, lo.PlainRig(pos, hier)), (none_v, none_f, lo.PlainRig([[0, 0, 0], [0, 1, 0]], [-1, 0])),
              (bv, bf, lo.PlainRig([[0, 0, 0]], [-1])), (bv, bf, lo.PlainRig([[0, 0, 0], [0.25, 0, 0]], [-1, 0])), (v16, none_f, lo.PlainRig(pos, hier))]
    out = labels.bone_ray_labels([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes])
    assert ops.calls == ["ray_cast", "ray_select", "ray_attention"] and len(out) == len(meshes)
    for (v, f, rig), (attn, fs, det) in zip(meshes, out):
        want = lo.labels(v, f, rig.pos, rig.hierarchy)
        assert attn.dtype == torch.float32 and fs.dtype == torch.float64 and same(attn, want["attn"]) and same(fs, want["featuresize"])
        for k in ("t", "face", "point", "kept", "ray_joint", "n_hit", "n_kept", "p20"):
            assert same(det[k], want[k]), k
    assert np.isnan(out[1][1].numpy()).all() and np.isnan(out[2][1].numpy()).all() and np.isnan(out[4][1].numpy()).all()      # NaN fill
    assert out[2][2]["t"].numel() == 0 and out[0][0].sum() > 0 and out[4][0].sum() == 0
    filled = labels.bone_ray_labels([bv], [bf], [meshes[2][2]], fill=-1.0)
    assert filled[0][1].tolist() == [-1.0]
    assert labels.bone_ray_labels([], [], []) == []


def test_lower_stages_and_refusals(ops):
    v, f, o, d, names = lo.on_grid_scene()
    for k in (0, 1, -1):
        t, face, point = labels.cast_rays(o, d, [0, len(o), len(o)], [v, v[:3]], [f, np.zeros((0, 3), dtype=np.int64)], orientation=k)
        want = lo.cast(o, d, v, f, k)
        assert same(t[0], want["t"]) and same(face[0], want["face"]) and same(point[0], want["point"]) and t[1].numel() == 0
    with pytest.raises(ValueError, match="outside its mesh"):
        labels.cast_rays(o, d, [0, len(o)], [v], [f + 20])
    with pytest.raises(ValueError, match="ray_ptr"):
        labels.cast_rays(o, d, [0, 3], [v], [f])
    with pytest.raises(ValueError, match="ray_ptr"):
        labels.cast_rays(o, d, [0, 5, 3, len(o)], [v, v, v], [f, f, f])
    with pytest.raises(ValueError, match="one segment per mesh"):
        labels.cast_rays(o, d, [0, len(o)], [v, v], [f, f])
    with pytest.raises(ValueError, match="orientation"):
        labels.cast_rays(o, d, [0, len(o)], [v], [f], orientation=2)
    t = np.concatenate([lo.hit_set(n, 1) for n in (0, 1, 5, 1024)])
    got = labels.select_hits(t, [0, 0, 1, 6, 1030], keep_factor=1.5, fill=7.0)
    want = lo.select(t, [0, 1, 5, 1024], 1.5, 7.0)
    for k in ("kept", "n_hit", "n_kept", "p20", "featuresize"):
        assert same(got[k], want[k]), k
    with pytest.raises(ValueError, match="1025 rays"):
        labels.select_hits(np.ones(1025), [0, 1025])
    with pytest.raises(ValueError, match="joint_ptr"):
        labels.select_hits(np.ones(5), [0, 4])
    with pytest.raises(ValueError, match="radius"):
        labels.attention([v], np.zeros((1, 3)), [1], [0, 1], radius=-0.02)


# ------------------------------------------------------------------------------------------------------------------------- files
def test_writers_and_readers_round_trip(tmp_path):
    rig = Rig.from_arrays(lo.torus_chain()[0], lo.torus_chain()[1], 0)
    fs = np.array([0.1, 1 / 3, np.nan, 1e-300, 2.5e10, 0.12345678901234567] * 2)
    name = str(tmp_path / "7.txt")
    labels.write_featuresize(name, rig, torch.from_numpy(fs))
    assert same(labels.read_featuresize(name, rig), fs)
    lines = open(name).read().splitlines()
    assert lines[0] == "joint_0 0.1" and lines[1] == "joint_1 " + repr(1 / 3) and lines[2] == "joint_2 nan" and len(lines) == 12
    table = {w[0]: float(w[1]) for w in (li.strip().split() for li in lines)}          # evaluate/eval_rigging.py:21-28
    assert same(np.array([table[n] for n in rig.names]), fs)
    with pytest.raises(ValueError, match="one value per joint"):
        labels.write_featuresize(name, rig, fs[:3])
    open(name, "w").write("joint_0 0.5\n")
    with pytest.raises(ValueError, match="joint_1"):
        labels.read_featuresize(name, rig)
    attn = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0])
    labels.write_attn(str(tmp_path / "7_attn.txt"), attn)
    assert open(str(tmp_path / "7_attn.txt")).read() == "0\n1\n1\n0\n1\n" and same(np.loadtxt(str(tmp_path / "7_attn.txt")), attn.double())


def test_a_sample_folder_reads_back_through_load_rig_sample(ops, tmp_path):
    v, f, pos, hier = lo.generated_scene(16)
    V = len(v)
    rng = np.random.default_rng(4)
    skins = rng.uniform(0, 1, (V, 12)) * (rng.uniform(0, 1, (V, 12)) < 0.3)
    skins[:, 0] += 0.1
    rig = Rig.from_arrays(pos, hier, 0, skins=skins)
    traj = np.stack([v + 0.01 * k for k in range(101)], 1)
    (attn, fs, _), = labels.bone_ray_labels([v], [f], [rig])
    (jid, offsets, gt_skin), = labels.rig_targets([traj[:, 0]], [rig])
    assert "nearest_point" in ops.calls and jid.dtype == torch.int64 and offsets.dtype == gt_skin.dtype == torch.float32
    stem = str(tmp_path / "12")
    np.save(stem + "_vtx_traj.npy", traj)
    labels.write_attn(stem + "_attn.txt", attn)
    edges = np.stack([np.arange(V), (np.arange(V) + 1) % V], 1)
    np.savetxt(stem + "_tpl_e.txt", edges, fmt="%d")
    np.savetxt(stem + "_geo_e.txt", edges, fmt="%d")
    rig.save(stem + "_rig.txt")
    bones, bone_names, leaf = skinning.get_bones(rig)
    k = formats.NUM_NEAREST_BONE
    bind = np.zeros((V, 3 * k))
    bind[:, 0::3] = rng.integers(0, len(bones), (V, k))
    bind[:, 1::3] = rng.uniform(0.1, 2.0, (V, k))
    skinning.write_skin_file(stem + "_skin.txt", bones, bone_names, bind, rng.uniform(0, 1, (V, k)))
    os.mkdir(str(tmp_path / "pred_flow"))
    for t in range(1, 6):
        np.save(str(tmp_path / "pred_flow" / f"12_{t}_pred_flow.npy"), np.zeros((V, 3), dtype=np.float32))
    data = formats.load_rig_sample(stem + "_vtx_traj.npy")
    assert same(data.mask, attn) and attn.sum() > 0                                     # bit-equal to the in-memory label
    saved = Rig(stem + "_rig.txt")                                                      # the file keeps 8 decimals of the joints
    (_, offsets_saved, gt_skin_saved), = labels.rig_targets([traj[:, 0]], [saved])
    assert same(data.offsets, offsets_saved) and same(data.gt_skin, gt_skin_saved)
    assert np.abs(offsets.numpy() - data.offsets.numpy()).max() < 1e-7
    labels.write_featuresize(stem + "_fs.txt", rig, fs)
    assert same(labels.read_featuresize(stem + "_fs.txt", saved), fs)


def test_evaluate_rigs_accepts_the_feature_sizes():
    import metrics_emulate as me
    from morig_amd import metrics
    v, f, pos, hier = lo.generated_scene(16)
    rigs = [Rig.from_arrays(pos, hier, 0), Rig.from_arrays(pos[:5], hier[:5], 0)]
    pred = np.concatenate([pos + 0.01, pos[:5] + 0.5])
    try:
        runtime._test_ops = le.LabelOps()
        fs = [o[1] for o in labels.bone_ray_labels([v, v], [f, f], rigs)]
        runtime._test_ops = me.MetricOps()
        res = metrics.evaluate_rigs(pred, [0, 12, 17], rigs, fs)
        assert res["hits"].tolist() == [12, 0] and res["recall"].tolist() == [1.0, 0.0]      # 0.017 < fs ~ 0.12 < 0.87
    finally:
        runtime._test_ops = None


# ------------------------------------------------------------------------------------------------------------------------- the host program
def test_boneray_core_under_the_sanitizers_equals_the_oracle(tmp_path):
    exe = str(tmp_path / "boneray_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "boneray_host_check.cpp"), "-o", exe], check=True)
    sets = [lo.hit_set(n, s) for s in (1, 2) for n in (0, 1, 2, 5, 6, 14, 1024)]
    sets += [np.full(6, np.inf), np.full(14, 0.25), np.array([np.inf, 0.5]), np.array([0.5, np.inf, 0.5, 0.5, np.inf, 0.25])]
    for keep_factor, fill in ((2.0, float("nan")), (0.5, -1.0)):
        t, counts = np.concatenate(sets), np.array([len(s) for s in sets], dtype=np.int32)
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("=iqdd", len(counts), len(t), keep_factor, fill))
            fh.write(counts.tobytes())
            fh.write(t.astype(np.float64).tobytes())
        done = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
        raw = open(dst, "rb").read()
        stats = np.frombuffer(raw[:32 * len(counts)], dtype=np.float64).reshape(-1, 4)
        kept = np.frombuffer(raw[32 * len(counts):], dtype=np.uint8)
        want = lo.select(t, counts, keep_factor, fill)
        assert same(kept, want["kept"]) and same(stats[:, 0], want["n_hit"].astype(np.float64)) and same(stats[:, 1], want["n_kept"].astype(np.float64))
        assert same(stats[:, 2], want["p20"]) and same(stats[:, 3], want["featuresize"])
        assert (want["n_kept"] < want["n_hit"]).any() and (want["n_hit"] == 0).any()
