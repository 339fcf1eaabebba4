"""csrc/motion_metrics.hip and morig_amd/motion_metrics.py on the device against tests/motion_metrics_oracle.py: every integer table and
every float64 ratio EXACTLY (the ratios are taken on the host from the integer tables, so they are the oracle's bits once the counts are),
on generated cases at the sizes the kernels branch on -- correspondences per pair around the wave (64) and the workgroup (256) and past
one workgroup, vertices per mesh around the wave, the workgroup's stride (256) and many strides, 1 / 10 / 32 bins -- and on the special
values: a distance equal to a tolerance, rows that a fused multiply-add would move across their tolerance, values equal to float32(t), a
constant mesh, a NaN, all-false and all-true labels. The key-frame flow error (float64 sums in the kernel's fixed order against numpy's):
1e-12 relative."""
import numpy as np
import pytest
import torch

import motion_metrics_oracle as mo
from morig_amd import motion_metrics as mm
from morig_amd.runtime import get_ops
from test_motion_metrics_host import CORR_KEYS, FEATURE_SHAPES, PR_KEYS, PR_SIZES, same, same_result

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = (0.02, 0.1, 0.2)
CORR_BATCHES = [[1025], [0], [0, 65], [255, 0], [0, 1, 63, 64, 65], [255, 0, 257, 1025, 64], [1, 63, 257, 65, 0]]
BIN_SETS = {1: mo.TOLERANCES[4:5], 10: mo.TOLERANCES, 32: list(np.linspace(0.01, 0.32, 32))}
THR_SETS = {1: mo.THRESHOLDS[3:4], 10: mo.THRESHOLDS, 32: np.linspace(0.0, 0.99, 32)}
_cache = {}
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def corr_case(sizes):
    key = ("corr", tuple(sizes))
    if key not in _cache:
        pairs = [mo.corr_pair(sum(sizes) + 7 * k, 300 + 11 * k, 130 + 5 * k, n, exact=EXACT) for k, n in enumerate(sizes)]
        pts, pb = mo.pack([p[0] for p in pairs])
        nnind, vb = mo.pack([p[1] for p in pairs])
        corr, cb = mo.pack([p[2].reshape(-1, 2) for p in pairs])
        args = dict(pts=dev(pts), corr_v2p=dev(corr), pts_batch=dev(pb), corr_v2p_batch=dev(cb), vtx_batch=dev(vb), num_graphs=len(pairs))
        _cache[key] = (pairs, args, dev(nnind))
    return _cache[key]


# --------------------------------------------------------------------------------------------------------------------- correspondences
@pytest.mark.parametrize("sizes", CORR_BATCHES, ids=lambda s: "-".join(map(str, s)))
def test_corr_accuracy_equals_the_oracle_exactly(sizes):
    pairs, args, nnind = corr_case(sizes)
    for n_bins in ((1, 10, 32) if len(sizes) == 5 else (10,)):
        tol = BIN_SETS[n_bins]
        got, want = mm.corr_accuracy(nnind=nnind, tolerances=tol, **args), mo.corr_accuracy(pairs, tol)
        print(f"pairs {sizes}, {n_bins} bins: hits {got['hits'].sum()} of {got['count'].sum()} x {n_bins}, n_valid {got['n_valid']}")
        assert same_result(got, want, CORR_KEYS) and got["n_valid"] == want["n_valid"]
    again = mm.corr_accuracy(nnind=nnind, **args)
    assert same_result(again, mm.corr_accuracy(nnind=nnind, **args), CORR_KEYS)                      # two runs, the same bits
    if sum(sizes) > 3:
        assert again["hits"][:, 0].sum() < again["hits"][:, -1].sum() < sum(sizes)                  # the data: hits and misses, more at 0.2


def test_a_distance_equal_to_its_tolerance_is_no_hit_and_no_product_is_fused():
    # rows 0 .. 2 of every pair of corr_pair(exact=EXACT) lie exactly 0.02, 0.1, 0.2 (as float32) apart: not a hit at that tolerance
    pairs, args, nnind = corr_case([65])
    pts, nn, corr = pairs[0]
    assert [float(d) for d in mo.corr_distance(pts, nn, corr[:3])] == [float(np.float32(t)) for t in EXACT]
    got = mm.corr_accuracy(nnind=nnind[:130], pts=args["pts"], corr_v2p=args["corr_v2p"][:3], pts_batch=args["pts_batch"],
                           corr_v2p_batch=args["corr_v2p_batch"][:3], vtx_batch=args["vtx_batch"])
    assert got["hits"][0].tolist() == [0, 1, 1, 1, 1, 2, 2, 2, 2, 2]
    # every row's tolerance is the larger of its plain and its fused distance: exactly one of the two arithmetics is below it
    pts, nn, corr, tol = mo.contraction_pair(32)
    zeros = lambda n: torch.zeros(n, dtype=torch.int64, device=DEV)
    got = mm.corr_accuracy(dev(pts), dev(corr), zeros(len(pts)), zeros(len(corr)), nnind=dev(nn), vtx_batch=zeros(len(nn)), tolerances=tol)
    want = mo.corr_hits(pts, nn, corr, tol)
    print("contraction probe: device", got["hits"][0].tolist(), "oracle", want.tolist())
    assert same(got["hits"][0], want)


def test_local_and_global_nn_give_the_same_tables_and_a_pair_alone_its_batch_counts():
    pairs, args, nnind = corr_case([255, 0, 257, 1025, 64])
    ops = get_ops()
    status = ops.loss_status(DEV)
    ptr_v, ptr_p, ptr_c = (ops.segment_ptr(args[k], 5, status) for k in ("vtx_batch", "pts_batch", "corr_v2p_batch"))
    tol = dev(mo.f32(mo.TOLERANCES))
    local = nnind.to(torch.int32)
    glob = (nnind + ptr_p.long()[args["vtx_batch"]]).to(torch.int32)
    a = ops.corr_hits(args["pts"], ptr_p, local, ptr_v, False, args["corr_v2p"], ptr_c, tol, status)
    b = ops.corr_hits(args["pts"], ptr_p, glob, ptr_v, True, args["corr_v2p"], ptr_c, tol, status)
    assert int(status) == 0 and torch.equal(a, b) and same(a.cpu().numpy(), mo.corr_accuracy(pairs)["hits"])
    for k in (0, 3):
        pts, nn, corr = pairs[k]
        zeros = lambda n: torch.zeros(n, dtype=torch.int64, device=DEV)
        alone = mm.corr_accuracy(dev(pts), dev(corr), zeros(len(pts)), zeros(len(corr)), nnind=dev(nn), vtx_batch=zeros(len(nn)))
        assert same(alone["hits"][0], a[k].cpu().numpy())


def test_an_index_outside_its_pair_raises_and_leaves_the_other_counts():
    pairs, args, nnind = corr_case([0, 1, 63, 64, 65])
    row = 1 + 63 + 5                                                                    # a row of pair 3
    corr = args["corr_v2p"].clone()
    corr[row, 1] = pairs[3][0].shape[0]                                                 # one past the pair's last point: pair 4's first
    with pytest.raises(mm.MotionMetricsInputError, match="MORIG_MOTION_ST_INDEX") as e:
        mm.corr_accuracy(nnind=nnind, **dict(args, corr_v2p=corr))
    without = list(pairs)
    without[3] = (pairs[3][0], pairs[3][1], np.delete(pairs[3][2], 5, axis=0))
    assert e.value.bits == 16 and same(e.value.result["hits"], mo.corr_accuracy(without)["hits"])
    unsorted = args["vtx_batch"].flip(0)
    with pytest.raises(mm.MotionMetricsInputError, match="MORIG_LOSS_ST_UNSORTED") as e:
        mm.corr_accuracy(nnind=nnind, **dict(args, vtx_batch=unsorted))
    assert e.value.result["hits"].sum() == 0


def test_feature_path_equals_the_float64_arg_max():
    feats = [mo.feature_pair(7 + k, v, p) for k, (v, p) in enumerate(FEATURE_SHAPES)]
    assert min(mo.similarity_gaps(f[0], f[1]).min() for f in feats) >= 1e-3                # a condition on the inputs: every vertex
    rng = np.random.default_rng(3)
    pts = [rng.random((p, 3)).astype(np.float32) for _, p in FEATURE_SHAPES]
    corr = [np.stack([rng.integers(0, v, n), rng.integers(0, p, n)], 1) for (v, p), n in zip(FEATURE_SHAPES, (4, 64, 257))]
    P, pb = mo.pack(pts)
    VF, vb = mo.pack([f[0] for f in feats])
    PF, _ = mo.pack([f[1] for f in feats])
    C, cb = mo.pack(corr)
    common = dict(pts=dev(P), corr_v2p=dev(C), pts_batch=dev(pb), corr_v2p_batch=dev(cb), vtx_batch=dev(vb), num_graphs=3)
    local = mm.nearest_points(dev(VF), dev(PF), dev(vb), dev(pb))
    assert local.dtype == torch.int64 and local.is_cuda and np.array_equal(local.cpu().numpy(), np.concatenate([f[2] for f in feats]))
    by_feature = mm.corr_accuracy(vtx_feature=dev(VF), pts_feature=dev(PF), **common)
    by_nnind = mm.corr_accuracy(nnind=local, **common)
    want = mo.corr_accuracy([(p, f[2], c) for p, f, c in zip(pts, feats, corr)])
    assert same_result(by_feature, want, CORR_KEYS) and same_result(by_nnind, want, CORR_KEYS)


# --------------------------------------------------------------------------------------------------------------------- attention
def attn_case(name):
    if name not in _cache:
        if name == "sizes":
            meshes = [mo.attn_mesh(100 + k, n) for k, n in enumerate(PR_SIZES)]
        else:
            kinds = ["at_threshold", "constant", "nan", "all_false", "all_true", "at_threshold", "nan"]
            meshes = [mo.attn_mesh(200 + k, n, kind) for k, (n, kind) in enumerate(zip([65, 257, 1025, 64, 63, 4097, 2], kinds))]
        pred, batch = mo.pack([m[0] for m in meshes])
        gt, _ = mo.pack([m[1] for m in meshes])
        _cache[name] = (meshes, dev(pred), dev(gt), dev(batch))
    return _cache[name]


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", ["sizes", "special"])
def test_pr_curve_equals_the_oracle_exactly(name, normalize):
    meshes, pred, gt, batch = attn_case(name)
    for n_bins, thr in THR_SETS.items():
        got = mm.pr_curve(pred[:, None], gt, batch, thresholds=thr, normalize=normalize)
        want = mo.pr_curve(meshes, thr, normalize)
        print(f"{name}, normalize={normalize}, {n_bins} bins: tp {got['tp'].sum()}, pp {got['pp'].sum()}, gp {got['gp'].tolist()}")
        assert same_result(got, want, PR_KEYS)
    assert same_result(got, mm.pr_curve(pred, gt, batch, thresholds=thr, normalize=normalize), PR_KEYS)          # two runs, the same bits
    k = 4 if name == "sizes" else 5
    alone = mm.pr_curve(dev(meshes[k][0]), dev(meshes[k][1]), torch.zeros(len(meshes[k][0]), dtype=torch.int64, device=DEV), thresholds=thr,
                        normalize=normalize)
    assert same(alone["tp"][0], got["tp"][k]) and same(alone["pp"][0], got["pp"][k]) and alone["gp"][0] == got["gp"][k]
    if name == "special":
        assert (got["pp"][1] == 0).all() == normalize and (got["pp"][2] == 0).all() == normalize       # constant, NaN: nothing once normalised
        assert got["gp"][3] == 0 and got["tp"][3].sum() == 0 and same(got["tp"][4], got["pp"][4])
        at = mm.pr_curve(pred, gt, batch, normalize=normalize)                        # mesh 0 holds every float32(t): equal is not above
        assert at["pp"][0].tolist() == mo.pr_curve(meshes[:1], normalize=normalize)["pp"][0].tolist()
    with pytest.raises(ValueError, match="mesh 9 has no vertices" if name == "sizes" else "mesh 7 has no vertices"):
        mm.pr_curve(pred, gt, batch, num_graphs=len(meshes) + 1)


# --------------------------------------------------------------------------------------------------------------------- flow, driver
@pytest.mark.parametrize("K", [1, 5])
def test_keyframe_flow_errors_against_the_float64_oracle(K):
    rng = np.random.default_rng(K)
    flows = [(rng.normal(0, 0.05, (n, 3 * K)).astype(np.float32), rng.normal(0, 0.05, (n, 3 * K)).astype(np.float32)) for n in (1, 65, 1025)]
    pred, batch = mo.pack([f[0] for f in flows])
    gt, _ = mo.pack([f[1] for f in flows])
    per_frame, per_mesh = mm.keyframe_flow_errors(dev(pred), dev(gt), dev(batch))
    want_frame, want_mesh = mo.keyframe_flow_errors(flows)
    rel = max(np.abs(per_frame / want_frame - 1).max(), np.abs(per_mesh / want_mesh - 1).max())
    print(f"keyframe_flow_errors K={K}: largest relative difference {rel:.3e}")
    assert per_frame.shape == (3, K) and per_mesh.shape == (3,) and rel <= 1e-12


def test_evaluate_motion_equals_the_three_calls():
    pairs, cargs, nnind = corr_case([0, 1, 63, 64, 65])
    meshes, pred, gt, batch = attn_case("sizes")
    rng = np.random.default_rng(9)
    flow = dict(pred_flow=dev(rng.normal(size=(len(pred), 15)).astype(np.float32)), gt_flow=dev(rng.normal(size=(len(pred), 15)).astype(np.float32)),
                batch=batch)
    attn = dict(pred=pred, gt=gt, batch=batch)
    res = mm.evaluate_motion(corr=dict(cargs, nnind=nnind), attn=attn, vismask=attn, flow=flow)
    assert same_result(res["corr"], mm.corr_accuracy(nnind=nnind, **cargs), CORR_KEYS) and same_result(res["attn"], mm.pr_curve(**attn), PR_KEYS)
    assert same_result(res["vismask"], mm.pr_curve(normalize=False, **attn), PR_KEYS)
    per_frame, per_mesh = mm.keyframe_flow_errors(**flow)
    assert same(res["flow"]["per_frame"], per_frame) and same(res["flow"]["per_mesh"], per_mesh)
    assert len(mm.format_motion_report(res).split("\n")) == 6
