"""Fixtures of the rig evaluation metrics (tests/golden/metrics_match.npz, metrics_skel.npz), made by the reference's own functions:
sample_skel, chamfer_dist, joint2bone_chamfer_dist and bone2bone_chamfer_dist of utils/eval_utils.py, on rigs that went through
formats.Rig.save and the reference's rig_parser.Info, imported from where the reference lies (oracle.shim.REFERENCE_ROOT). Nothing of the
reference is written into the repository: only inputs and recorded results. The matching block of eval_rig (evaluate/eval_rigging.py:
113-120) is inline in a module that imports open3d and cv2; it is computed here from its statement: the distance matrix with rows =
ground truth, scipy's linear_sum_assignment, hits = sum(d < fs[row]), IoU = 2 hits / (n_pred + n_gt), precision, recall.

  metrics_match   one batch of the (n_gt, n_pred) shapes SHAPES and one mesh without predicted joints: ground-truth joints uniform in the
                  unit box, predictions = a subset perturbed by N(0, 0.03^2) plus uniform strays, feature sizes U(0.02, 0.08). Stored:
                  the matching, matched distances, hits, IoU, precision, recall, the reference's chamfer_dist per mesh, the means over
                  the valid meshes and the report text. Also a TIE case (joints on an integer lattice line: small-integer costs, many
                  equal optima) with its optimal total.
  metrics_skel    pairs of rigs whose bone-sample sets run from a handful of points to past one LDS tile of nearest_distance (1024):
                  a star around the origin with a zero-length bone and axis-aligned bones whose len / 0.005 is exactly k + 0.5 for even
                  and odd k (and the near miss 3.5), then random trees. Joint coordinates are multiples of 1 / 256 (exact in %.8f, and
                  (p - parent) + parent == p in Rig's forward pass) except the star's. Stored: the reference's samples per rig, CD-J2B,
                  CD-B2B, and for the meshes EVAL_MESHES the evaluation with the first rig as the prediction.

Conditions enforced here (a seed that misses one is skipped, the search fails rather than write such a fixture) and re-asserted by
tests/test_metrics_oracle.py: every parity case has a UNIQUE optimum (forbid each matched pair in turn and re-solve: the best such total
exceeds the optimum by more than GAP = 1e-6) and every matched distance differs from its feature size by more than MARGIN = 1e-9; no
sample set has more than 4096 points (the summation bound of the tests); the rigs read back through Info hold exactly the stored joints.

Run from the repository root:  python tools/make_metrics_golden.py
"""
import os
import sys
import tempfile

import numpy as np
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (save, OUT)
import metrics_oracle as mo                                                    # noqa: E402
from morig_amd import formats                                                  # noqa: E402

SHAPES = [(1, 1), (1, 5), (5, 1), (7, 7), (24, 31), (33, 20), (64, 65), (65, 64), (96, 96), (12, 0)]
GAP, MARGIN, MAX_SAMPLES = 1e-6, 1e-9, 4096
HALF_STEPS = [1.5, 2.5, 4.5, 5.5, 6.5, 7.5]                 # len / 0.005 is exactly k + 0.5 in float64 for these
NEAR_MISS = 3.5
TREES = [(4, 5, 0.03), (5, 3, 0.0625), (12, 10, 0.5), (14, 20, 1.0), (9, 16, 1.0)]      # joints of rig a, of rig b, box edge
EVAL_MESHES = [1, 2, 3, 4, 5]


def reference():
    if shim.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, shim.REFERENCE_ROOT)
    return __import__("utils.eval_utils", fromlist=["sample_skel"]), __import__("utils.rig_parser", fromlist=["Info"])


def inline_scores(pred, gt, fs):
    """the matching block of eval_rig from its statement"""
    d = np.sqrt(np.sum((pred[np.newaxis, ...] - gt[:, np.newaxis, :]) ** 2, axis=2))
    row, col = linear_sum_assignment(d)
    hits = np.sum(d[row, col] < fs[row])
    return dict(d=d, row=row, col=col, dist=d[row, col], hits=int(hits), iou=2 * hits / (len(pred) + len(gt)), precision=hits / len(pred),
                recall=hits / len(gt))


def conditions(s, fs):
    return mo.assignment_gap(s["d"]), mo.threshold_margin(s["dist"], fs[s["row"]])


def report(ref_means):
    return "\n".join(["\tJ2J_chamfer_distance {:.03f}%".format(ref_means[0] * 100), "\tjoint_IoU {:.03f}%".format(ref_means[1] * 100),
                      "\tjoint_precision {:.03f}%".format(ref_means[2] * 100), "\tjoint_recall {:.03f}%".format(ref_means[3] * 100)])


def make_match(eu):
    meshes, seed = [], 0
    for n_gt, n_pred in SHAPES:
        while True:
            seed += 1
            rng = np.random.default_rng(1000 + seed)
            gt = rng.random((n_gt, 3))
            fs = rng.uniform(0.02, 0.08, n_gt)
            near = rng.permutation(n_gt)[:min(n_gt, n_pred)]
            pred = np.concatenate([gt[near] + rng.normal(0.0, 0.03, (len(near), 3)), rng.random((n_pred - len(near), 3))], axis=0)
            pred = pred[rng.permutation(n_pred)]
            if n_pred == 0:
                meshes.append(dict(gt=gt, pred=pred, fs=fs, seed=1000 + seed, gap=None, margin=None, s=None))
                break
            s = inline_scores(pred, gt, fs)
            gap, margin = conditions(s, fs)
            if gap > GAP and margin > MARGIN:
                meshes.append(dict(gt=gt, pred=pred, fs=fs, seed=1000 + seed, gap=float(gap), margin=float(margin), s=s))
                break
    valid = [m for m in meshes if m["s"] is not None]
    totals = np.zeros(4)
    j2j = np.full(len(meshes), np.nan)
    for b, m in enumerate(meshes):
        if m["s"] is None:
            continue
        j2j[b] = eu.chamfer_dist(m["pred"], m["gt"])
        totals += np.array([j2j[b], m["s"]["iou"], m["s"]["precision"], m["s"]["recall"]])         # in mesh order, as eval_rig adds them
    means = totals / (len(meshes) - (len(meshes) - len(valid)))
    cat = lambda k, dt=np.float64: np.concatenate([np.asarray(m["s"][k], dtype=dt) for m in valid])
    ptr = lambda k: np.concatenate([[0], np.cumsum([len(m[k]) for m in meshes])]).astype(np.int32)
    # the tie case: joints on an integer lattice line
    tie_gt = np.array([[x, 0.0, 0.0] for x in (0, 1, 2, 3, 4, 5)], dtype=np.float64)
    tie_pred = np.array([[x, 0.0, 0.0] for x in (0, 0, 2, 2, 4, 4, 6, 6)], dtype=np.float64)
    ts = inline_scores(tie_pred, tie_gt, np.full(len(tie_gt), 0.5))
    assert mo.assignment_gap(ts["d"]) == 0.0 and np.all(ts["d"] == np.round(ts["d"]))
    meta = dict(shapes=SHAPES, seeds=[m["seed"] for m in meshes], gaps=[m["gap"] for m in meshes], margins=[m["margin"] for m in meshes],
                report=report(means), num_invalid=len(meshes) - len(valid), tie_total=float(ts["dist"].sum()))
    msg.save("metrics_match", meta, gt=np.concatenate([m["gt"] for m in meshes]), gt_ptr=ptr("gt"),
             pred=np.concatenate([m["pred"] for m in meshes]), pred_ptr=ptr("pred"), fs=np.concatenate([m["fs"] for m in meshes]),
             row_ind=cat("row", np.int32), col_ind=cat("col", np.int32), dist=cat("dist"),
             match_ptr=np.concatenate([[0], np.cumsum([min(s) for s in SHAPES])]).astype(np.int32),
             hits=np.array([m["s"]["hits"] if m["s"] else 0 for m in meshes], dtype=np.int32),
             iou=np.array([m["s"]["iou"] if m["s"] else np.nan for m in meshes]),
             precision=np.array([m["s"]["precision"] if m["s"] else np.nan for m in meshes]),
             recall=np.array([m["s"]["recall"] if m["s"] else np.nan for m in meshes]), chamfer_j2j=j2j, means=means, tie_gt=tie_gt,
             tie_pred=tie_pred)
    print("  smallest gap", min(m["gap"] for m in valid), "smallest margin", min(m["margin"] for m in valid))


def through_info(rig, rp, tmp):
    """Rig.save, then the reference's Info: the skeleton the reference's functions take; its joints must be the rig's, to the bit"""
    path = os.path.join(tmp, "rig.txt")
    rig.save(path)
    info = rp.Info(path)
    back = formats.Rig(path)
    assert np.array_equal(back.pos, rig.pos) and np.array_equal(back.hierarchy, rig.hierarchy), "the rig does not survive its file"
    for name, p in info.joint_pos.items():
        assert np.array_equal(np.array(p), rig.pos[rig.names.index(name)])
    return info


def star_rig():
    """root at the origin; children on the axes at the half-step lengths (both signs), the near miss, and one zero-length bone"""
    pos, lengths = [[0.0, 0.0, 0.0]], []
    for i, k in enumerate(HALF_STEPS + [NEAR_MISS]):
        length = float("{:.8f}".format(k * 0.005))
        lengths.append(length)
        p = [0.0, 0.0, 0.0]
        p[i % 3] = length if i % 2 == 0 else -length
        pos.append(p)
    pos.append([0.0, 0.0, 0.0])                                                 # zero-length bone: one sample
    pos = np.array(pos, dtype=np.float64)
    for k, length in zip(HALF_STEPS, lengths):
        assert length / 0.005 == k and np.round(length / 0.005) == (np.floor(k) if np.floor(k) % 2 == 0 else np.ceil(k)), (k, length)
    assert lengths[-1] / 0.005 != NEAR_MISS
    return formats.Rig.from_arrays(pos, [-1] + [0] * (len(pos) - 1), 0)


def random_tree(rng, n, edge):
    pos = rng.integers(0, int(round(edge * 256)) + 1, (n, 3)) / 256.0
    hier = [-1] + [int(rng.integers(0, j)) for j in range(1, n)]
    return formats.Rig.from_arrays(pos, hier, 0)


def make_skel(eu, rp):
    rng = np.random.default_rng(77)
    with tempfile.TemporaryDirectory() as tmp:
        pairs = [(star_rig(), random_tree(rng, 3, 0.02))]
        fss, evals, seed = [None], [None], 0
        for na, nb, edge in TREES:
            while True:
                seed += 1
                r = np.random.default_rng(2000 + seed)
                a, b = random_tree(r, na, edge), random_tree(r, nb, edge)
                fs = r.uniform(0.02, 0.08, nb) * max(edge, 0.25)
                s = inline_scores(a.pos, b.pos, fs)
                gap, margin = conditions(s, fs)
                n_max = max(len(mo.sample_skel(a)), len(mo.sample_skel(b)))
                if gap > GAP and margin > MARGIN and n_max <= MAX_SAMPLES and len(np.unique(np.concatenate([a.pos, b.pos]), axis=0)) == na + nb:
                    pairs.append((a, b))
                    fss.append(fs)
                    evals.append(dict(s=s, gap=float(gap), margin=float(margin), seed=2000 + seed))
                    break
        arrs, meta = {}, dict(n=len(pairs), eval_meshes=EVAL_MESHES, counts=[], gaps=[], margins=[])
        j2b, b2b, j2j = [], [], []
        for i, (a, b) in enumerate(pairs):
            ia, ib = through_info(a, rp, tmp), through_info(b, rp, tmp)
            for tag, rig, info in (("a", a, ia), ("b", b, ib)):
                samples = eu.sample_skel(info)
                assert len(samples) <= MAX_SAMPLES
                arrs[f"pos_{tag}{i}"], arrs[f"hier_{tag}{i}"], arrs[f"samples_{tag}{i}"] = rig.pos, np.asarray(rig.hierarchy, dtype=np.int32), samples
            meta["counts"].append([len(arrs[f"samples_a{i}"]), len(arrs[f"samples_b{i}"])])
            j2b.append(eu.joint2bone_chamfer_dist(ia, ib))
            b2b.append(eu.bone2bone_chamfer_dist(ia, ib))
            j2j.append(eu.chamfer_dist(a.pos, b.pos))
            if fss[i] is not None:
                arrs[f"fs{i}"] = fss[i]
                meta["gaps"].append(evals[i]["gap"])
                meta["margins"].append(evals[i]["margin"])
        assert max(max(c) for c in meta["counts"]) > 1024 and min(min(c) for c in meta["counts"]) < 64
        assert [i for i in range(len(pairs)) if fss[i] is not None] == EVAL_MESHES
        # the evaluation of EVAL_MESHES (rig a = prediction) and of one more mesh without predicted joints
        totals = np.zeros(6)
        for i in EVAL_MESHES:
            s = evals[i]["s"]
            totals += np.array([j2j[i], s["iou"], s["precision"], s["recall"], j2b[i], b2b[i]])
        means = totals / (len(EVAL_MESHES) + 1 - 1)
        meta["report"] = report(means)
        msg.save("metrics_skel", meta, chamfer_j2b=np.array(j2b), chamfer_b2b=np.array(b2b), chamfer_j2j=np.array(j2j), eval_means=means,
                 eval_hits=np.array([evals[i]["s"]["hits"] for i in EVAL_MESHES], dtype=np.int32), **arrs)
        print("  sample counts", meta["counts"])


def main():
    eu, rp = reference()
    make_match(eu)
    make_skel(eu, rp)
    total = sum(os.path.getsize(os.path.join(msg.OUT, f)) for f in os.listdir(msg.OUT) if f.startswith("metrics_"))
    assert total <= 600 << 10, total
    print("  metrics fixtures:", total, "bytes")


if __name__ == "__main__":
    main()
