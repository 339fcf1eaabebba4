"""CPU: the host logic of morig_amd/motion_metrics.py on an emulated op layer (tests/motion_metrics_emulate.py through
``runtime._test_ops``): ragged packing, nnind against the feature path, the refusals, the status word, NaN handling and n_valid, the
report; and csrc/curve_core.h as the stand-alone program tools/curve_host_check.cpp, built with the address and undefined-behaviour
sanitizers and run as a program against tests/motion_metrics_oracle.py."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import motion_metrics_emulate as me
import motion_metrics_oracle as mo
from morig_amd import motion_metrics as mm
from morig_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORR_SIZES = [0, 1, 63, 64, 65, 255, 257, 1025]
PR_SIZES = [1, 2, 63, 64, 65, 256, 257, 1025, 4097]
FEATURE_SHAPES = [(5, 7), (64, 65), (130, 257)]


@pytest.fixture()
def ops():
    emu = me.MotionOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(got, want, keys):
    return all(same(got[k], want[k]) for k in keys)


CORR_KEYS = ("hits", "count", "acc", "curve")
PR_KEYS = ("tp", "pp", "gp", "precision", "recall", "mean_precision", "mean_recall")


def corr_batch(sizes, seed=0):
    pairs = [mo.corr_pair(seed + 10 * k, 40 + 3 * k, 30 + 2 * k, n, exact=(0.02, 0.1)) for k, n in enumerate(sizes)]
    pts, pb = mo.pack([p[0] for p in pairs])
    nnind, vb = mo.pack([p[1] for p in pairs])
    corr, cb = mo.pack([p[2].reshape(-1, 2) for p in pairs])
    args = dict(pts=torch.from_numpy(pts), corr_v2p=torch.from_numpy(corr), pts_batch=torch.from_numpy(pb), corr_v2p_batch=torch.from_numpy(cb),
                vtx_batch=torch.from_numpy(vb), num_graphs=len(pairs))
    return pairs, args, torch.from_numpy(nnind)


# --------------------------------------------------------------------------------------------------------------------- correspondences
def test_corr_accuracy_of_a_ragged_batch_equals_the_loop(ops):
    pairs, args, nnind = corr_batch([5, 0, 64, 1, 0])
    got = mm.corr_accuracy(nnind=nnind, **args)
    want = mo.corr_accuracy(pairs)
    assert same_result(got, want, CORR_KEYS) and got["n_valid"] == 3 and ops.calls == ["corr_hits"]
    assert np.isnan(got["acc"][1]).all() and np.isnan(got["acc"][4]).all() and not np.isnan(got["curve"]).any()
    assert got["hits"].dtype == np.int64 and got["acc"].dtype == np.float64 and got["hits"].shape == (5, 10)
    one = mm.corr_accuracy(nnind=nnind, **dict(args, num_graphs=None))                  # num_graphs read from the batch vector
    assert same_result(one, want, CORR_KEYS)
    nothing = mm.corr_accuracy(nnind=nnind[:0], pts=args["pts"][:0], corr_v2p=args["corr_v2p"][:0], pts_batch=args["pts_batch"][:0],
                               corr_v2p_batch=args["corr_v2p_batch"][:0], vtx_batch=args["vtx_batch"][:0], num_graphs=2)
    assert nothing["n_valid"] == 0 and np.isnan(nothing["curve"]).all() and nothing["hits"].sum() == 0


def test_other_tolerances_and_the_bin_limit(ops):
    pairs, args, nnind = corr_batch([65, 3])
    for tol in ([0.05], list(np.linspace(0.01, 0.3, 32))):
        assert same_result(mm.corr_accuracy(nnind=nnind, tolerances=tol, **args), mo.corr_accuracy(pairs, tol), CORR_KEYS)
    with pytest.raises(ValueError, match="32"):
        mm.corr_accuracy(nnind=nnind, tolerances=list(np.linspace(0.01, 0.3, 33)), **args)
    with pytest.raises(ValueError, match="32"):
        mm.pr_curve(torch.rand(4), torch.ones(4), torch.zeros(4, dtype=torch.int64), thresholds=[])


@pytest.mark.parametrize("shape", FEATURE_SHAPES)
def test_feature_generator_separates_every_vertex(shape):
    vtx_f, pts_f, best = mo.feature_pair(shape[0], *shape)
    gaps = mo.similarity_gaps(vtx_f, pts_f)
    assert gaps.min() >= 1e-3 and np.allclose(np.linalg.norm(vtx_f.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.array_equal(best, (vtx_f.astype(np.float64) @ pts_f.astype(np.float64).T).argmax(axis=1))


def test_feature_path_equals_the_nnind_path(ops):
    feats = [mo.feature_pair(7 + k, v, p) for k, (v, p) in enumerate(FEATURE_SHAPES)]
    rng = np.random.default_rng(3)
    pts = [rng.random((p, 3)).astype(np.float32) for _, p in FEATURE_SHAPES]
    corr = [np.stack([rng.integers(0, v, n), rng.integers(0, p, n)], 1) for (v, p), n in zip(FEATURE_SHAPES, (4, 64, 257))]
    P, pb = mo.pack(pts)
    VF, vb = mo.pack([f[0] for f in feats])
    PF, _ = mo.pack([f[1] for f in feats])
    C, cb = mo.pack(corr)
    t = torch.from_numpy
    common = dict(pts=t(P), corr_v2p=t(C), pts_batch=t(pb), corr_v2p_batch=t(cb), vtx_batch=t(vb), num_graphs=3)
    local = mm.nearest_points(t(VF), t(PF), t(vb), t(pb))
    assert local.dtype == torch.int64 and np.array_equal(local.numpy(), np.concatenate([f[2] for f in feats]))
    by_feature = mm.corr_accuracy(vtx_feature=t(VF), pts_feature=t(PF), **common)
    by_nnind = mm.corr_accuracy(nnind=local, **common)
    want = mo.corr_accuracy([(p, f[2], c) for p, f, c in zip(pts, feats, corr)])
    assert same_result(by_feature, want, CORR_KEYS) and same_result(by_nnind, want, CORR_KEYS)
    assert ops.calls == ["cosine_nn", "cosine_nn", "corr_hits", "corr_hits"]


def test_corr_refusals(ops):
    pairs, args, nnind = corr_batch([5, 3])
    f = torch.zeros(nnind.numel(), 64)
    pf = torch.zeros(args["pts"].shape[0], 64)
    with pytest.raises(ValueError, match="not both"):
        mm.corr_accuracy(nnind=nnind, vtx_feature=f, pts_feature=pf, **args)
    with pytest.raises(ValueError, match="give nnind, or both"):
        mm.corr_accuracy(**args)
    with pytest.raises(ValueError, match="give nnind, or both"):
        mm.corr_accuracy(vtx_feature=f, **args)
    with pytest.raises(ValueError, match="vtx_batch"):
        mm.corr_accuracy(nnind=nnind, **dict(args, vtx_batch=None))
    with pytest.raises(ValueError, match="width 32.*width 64"):
        mm.corr_accuracy(vtx_feature=f[:, :32], pts_feature=pf[:, :32], **args)
    with pytest.raises(ValueError, match="width 64"):
        mm.nearest_points(torch.zeros(3, 128), torch.zeros(4, 128), torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="float32"):
        mm.corr_accuracy(nnind=nnind, **dict(args, pts=args["pts"].double()))
    with pytest.raises(ValueError, match="one entry per vertex"):
        mm.corr_accuracy(nnind=nnind[:-1], **args)


def test_bad_data_arrives_through_the_status_word(ops):
    pairs, args, nnind = corr_batch([5, 3, 4])
    clean = mm.corr_accuracy(nnind=nnind, **args)
    # one correspondence row names a point outside its pair: that row counts nothing, the rest is unchanged
    corr = args["corr_v2p"].clone()
    corr[6, 1] = pairs[1][0].shape[0]                                                   # pair 1, its second row
    with pytest.raises(mm.MotionMetricsInputError, match="MORIG_MOTION_ST_INDEX") as e:
        mm.corr_accuracy(nnind=nnind, **dict(args, corr_v2p=corr))
    without = [pairs[0], (pairs[1][0], pairs[1][1], np.delete(pairs[1][2], 1, axis=0)), pairs[2]]
    assert same(e.value.result["hits"], mo.corr_accuracy(without)["hits"]) and same(e.value.result["hits"][[0, 2]], clean["hits"][[0, 2]])
    assert e.value.result["count"].tolist() == [5, 3, 4] and e.value.bits == 16
    bad_nn = nnind.clone()
    bad_nn[int(pairs[0][2][0, 0])] = -1                                                 # a vertex some row of pair 0 names
    with pytest.raises(mm.MotionMetricsInputError, match="outside its pair"):
        mm.corr_accuracy(nnind=bad_nn, **args)
    unsorted = args["pts_batch"].clone()
    unsorted[[0, -1]] = unsorted[[-1, 0]]
    with pytest.raises(mm.MotionMetricsInputError, match="MORIG_LOSS_ST_UNSORTED") as e:
        mm.corr_accuracy(nnind=nnind, **dict(args, pts_batch=unsorted))
    assert e.value.result["hits"].sum() == 0
    with pytest.raises(mm.MotionMetricsInputError, match="MORIG_LOSS_ST_SEGMENT"):
        mm.corr_accuracy(nnind=nnind, **dict(args, num_graphs=2))
    with pytest.raises(mm.MotionMetricsInputError, match="not sorted"):
        mm.pr_curve(torch.rand(4), torch.ones(4), torch.tensor([0, 1, 0, 1]))
    with pytest.raises(mm.MotionMetricsInputError, match="not sorted"):
        mm.keyframe_flow_errors(torch.rand(4, 3), torch.rand(4, 3), torch.tensor([1, 1, 0, 0]))
    assert issubclass(mm.MotionMetricsInputError, ValueError)


# --------------------------------------------------------------------------------------------------------------------- attention
def test_pr_curve_of_a_ragged_batch_equals_the_loop(ops):
    kinds = ["random", "at_threshold", "constant", "nan", "all_false", "all_true", "random"]
    meshes = [mo.attn_mesh(k, n, kind) for k, (n, kind) in enumerate(zip([65, 40, 7, 130, 3, 64, 1], kinds))]
    pred, batch = mo.pack([m[0] for m in meshes])
    gt, _ = mo.pack([m[1] for m in meshes])
    for normalize in (True, False):
        got = mm.pr_curve(torch.from_numpy(pred)[:, None], torch.from_numpy(gt), torch.from_numpy(batch), normalize=normalize)
        want = mo.pr_curve(meshes, normalize=normalize)
        assert same_result(got, want, PR_KEYS)
        assert (got["pp"][2] == 0).all() == normalize and (got["pp"][3] == 0).all() == normalize       # constant mesh, NaN mesh: nothing when normalised
        assert (got["tp"][4] == 0).all() and got["gp"][4] == 0 and same(got["tp"][5], got["pp"][5]) and got["gp"][5] == 64
    assert got["precision"].dtype == np.float64 and got["tp"].dtype == np.int64 and got["tp"].shape == (7, 10)
    assert same_result(mm.pr_curve(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(batch), thresholds=[0.25]),
                       mo.pr_curve(meshes, [0.25]), PR_KEYS)


def test_pr_curve_refusals(ops):
    pred, gt = torch.rand(6), torch.ones(6)
    with pytest.raises(ValueError, match="mesh 1 has no vertices"):
        mm.pr_curve(pred, gt, torch.tensor([0, 0, 0, 2, 2, 2]))
    with pytest.raises(ValueError, match="mesh 2 has no vertices"):
        mm.pr_curve(pred, gt, torch.tensor([0, 0, 0, 1, 1, 1]), num_graphs=3)
    with pytest.raises(ValueError, match="float32"):
        mm.pr_curve(pred.double(), gt, torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError, match="one label per vertex"):
        mm.pr_curve(pred, gt[:5], torch.zeros(6, dtype=torch.int64))


# --------------------------------------------------------------------------------------------------------------------- flow, driver, report
def test_flow_errors_and_the_driver(ops):
    rng = np.random.default_rng(5)
    flows = [(rng.normal(size=(n, 15)).astype(np.float32), rng.normal(size=(n, 15)).astype(np.float32)) for n in (1, 17, 65)]
    pred, batch = mo.pack([f[0] for f in flows])
    gt, _ = mo.pack([f[1] for f in flows])
    per_frame, per_mesh = mm.keyframe_flow_errors(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(batch))
    want_frame, want_mesh = mo.keyframe_flow_errors(flows)
    assert per_frame.shape == (3, 5) and np.allclose(per_frame, want_frame, rtol=1e-12, atol=0) and np.allclose(per_mesh, want_mesh, rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match=r"\[V, 3 K\]"):
        mm.keyframe_flow_errors(torch.zeros(4, 5), torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64))
    pairs, cargs, nnind = corr_batch([5, 0, 9])
    meshes = [mo.attn_mesh(k, n) for k, n in enumerate((12, 30))]
    apred, abatch = mo.pack([m[0] for m in meshes])
    agt, _ = mo.pack([m[1] for m in meshes])
    attn = dict(pred=torch.from_numpy(apred), gt=torch.from_numpy(agt), batch=torch.from_numpy(abatch))
    flow = dict(pred_flow=torch.from_numpy(pred), gt_flow=torch.from_numpy(gt), batch=torch.from_numpy(batch))
    res = mm.evaluate_motion(corr=dict(cargs, nnind=nnind), attn=attn, vismask=attn, flow=flow)
    assert same_result(res["corr"], mo.corr_accuracy(pairs), CORR_KEYS) and same_result(res["attn"], mo.pr_curve(meshes), PR_KEYS)
    assert same_result(res["vismask"], mo.pr_curve(meshes, normalize=False), PR_KEYS) and same(res["flow"]["per_mesh"], per_mesh)
    assert res["flow"]["mean"] == ((per_mesh[0] + per_mesh[1]) + per_mesh[2]) / 3
    assert list(mm.evaluate_motion(attn=attn)) == ["attn"]
    with pytest.raises(ValueError, match="at least one"):
        mm.evaluate_motion()
    lines = mm.format_motion_report(res).split("\n")
    assert len(lines) == 6 and lines[0].startswith("\tcorr_accuracy(%) over 2 of 3 pairs at tolerances 0.02 0.04") and lines[0].count(" ") > 20
    assert lines[1].startswith("\tattn_precision over 2 meshes at thresholds 0.0 0.1") and lines[4].startswith("\tvismask_recall")
    assert lines[0].endswith(" ".join("{:.03f}".format(v) for v in res["corr"]["curve"]))
    assert lines[5] == "\tkeyframe_flow_error over 3 meshes and 5 key frames: {:.06f}".format(res["flow"]["mean"])


# --------------------------------------------------------------------------------------------------------------------- the host program
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("curve") / "curve_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "curve_host_check.cpp"), "-o", path], check=True)
    return path


def run_program(exe, tmp_path, payload, n_out):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(payload)
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-2000:])
    out = np.fromfile(dst, dtype=np.int64)
    assert len(out) == n_out
    return out


def test_curve_core_under_the_sanitizers_equals_the_oracle(exe, tmp_path):
    bin_sets = [mo.TOLERANCES[:1], mo.TOLERANCES, list(np.linspace(0.01, 0.32, 32))]
    for k, n in enumerate(CORR_SIZES):
        pts, nnind, corr = mo.corr_pair(40 + k, 50 + k, 33 + k, n, exact=(0.02, 0.1, 0.2))
        for base in (0, 1000):
            for tol in bin_sets:
                bins = mo.f32(tol)
                payload = struct.pack("=ii", 0, len(bins)) + bins.tobytes() + struct.pack("=iiii", len(pts), len(nnind), len(corr), base)
                payload += pts.tobytes() + (nnind + base).astype(np.int32).tobytes() + corr.astype(np.int64).tobytes()
                out = run_program(exe, tmp_path, payload, len(bins) + 1)
                assert same(out[:-1], mo.corr_hits(pts, nnind, corr, tol)) and out[-1] == 0
    # rows with an index outside the pair count nothing and are reported
    pts, nnind, corr = mo.corr_pair(1, 20, 10, 8)
    bad = corr.copy()
    bad[0, 0], bad[3, 1], bad[5, 0] = 10, -1, -7
    nn_bad = nnind.copy()
    nn_bad[int(corr[7, 0])] = 20
    keep = [r for r in (1, 2, 4, 6) if corr[r, 0] != corr[7, 0]]
    bins = mo.f32(mo.TOLERANCES)
    payload = struct.pack("=ii", 0, 10) + bins.tobytes() + struct.pack("=iiii", 20, 10, 8, 0) + pts.tobytes() + nn_bad.astype(np.int32).tobytes()
    out = run_program(exe, tmp_path, payload + bad.astype(np.int64).tobytes(), 11)
    assert out[-1] == 8 - len(keep) and same(out[:-1], mo.corr_hits(pts, nnind, corr[keep], mo.TOLERANCES))
    # the attention counts, with the special values
    kinds = ["random", "at_threshold", "constant", "nan", "all_false", "all_true"]
    for k, n in enumerate(PR_SIZES):
        for kind in (kinds if n in (2, 65, 257) else kinds[:2]):
            pred, gt = mo.attn_mesh(k, n, kind)
            for normalize in (1, 0):
                for thr in (mo.THRESHOLDS[:1], mo.THRESHOLDS, np.linspace(0.0, 0.99, 32)):
                    bins = mo.f32(thr)
                    payload = struct.pack("=ii", 1, len(bins)) + bins.tobytes() + struct.pack("=ii", n, normalize) + pred.tobytes()
                    out = run_program(exe, tmp_path, payload + (gt != 0).astype(np.uint8).tobytes(), 2 * len(bins) + 1)
                    tp, pp, gp = mo.pr_counts(pred, gt, thr, bool(normalize))
                    assert same(out[:len(bins)], tp) and same(out[len(bins):-1], pp) and out[-1] == gp, (n, kind, normalize)
