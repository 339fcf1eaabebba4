"""The fixture of the motion-stage evaluation (tests/golden/motion_metrics.npz), made by the reference's own statements, compiled from the
reference's files at generation time (as tools/make_skin_golden.py does for post_filter); nothing of the reference is written into the
repository, only inputs and recorded results:

  evaluate/eval_corr.py     the assignment of ratio_list and lines 17-23 (pred_pos .. the loop over the tolerances), per pair
  evaluate/eval_attn.py     line 21 (the normalisation) and lines 32-34 of the loop of line 31 (the predicted positives, precision, recall),
                            per mesh, with np.bool mapped to bool
  evaluate/eval_deform.py   line 18 (the mean vertex distance of one key frame), per mesh and key frame

Recorded next to them: the integer counts (hits from acc, checked to reproduce it to the bit; tp, pp from the reference's own boolean
array) and the means in mesh order.

Conditions asserted here and again by tests/test_motion_metrics_oracle.py: every normalised attention value is more than MARGIN = 1e-6
away from every threshold that float32 does not hold exactly (0.0 is exact: float32 and float64 agree on it for every value) -- then the
float64 comparison of the numpy that runs this tool and the float32 comparison of the reference's numpy 1.21 give the same counts; every
correspondence distance is more than MARGIN away from every tolerance.

Run from the repository root:  python tools/make_motion_metrics_golden.py
"""
import ast
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (save)
import motion_metrics_oracle as mo                                             # noqa: E402

MARGIN = 1e-6
CORR_PAIRS = [(50, 40, 30), (300, 200, 257), (7, 5, 1), (120, 100, 64), (9, 6, 0)]          # points, vertices, correspondences
ATTN_MESHES = [2, 65, 300, 1025]
FLOW_MESHES, KEYFRAMES = [1, 65, 1025], 5


def _statements(path, keep):
    """the statements of a reference file (at any depth) that ``keep`` accepts, in file order, compiled"""
    tree = ast.parse(open(path).read())
    picked = [n for n in ast.walk(tree) if isinstance(n, ast.stmt) and keep(n)]
    picked.sort(key=lambda n: n.lineno)
    return compile(ast.Module(body=picked, type_ignores=[]), path, "exec")


def corr_code():
    path = os.path.join(shim.REFERENCE_ROOT, "evaluate", "eval_corr.py")
    tolerances = _statements(path, lambda n: isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "ratio_list")
    body = _statements(path, lambda n: (isinstance(n, ast.Assign) and 17 <= n.lineno <= 19) or (isinstance(n, ast.For) and n.lineno == 20))
    return tolerances, body


def attn_code():
    path = os.path.join(shim.REFERENCE_ROOT, "evaluate", "eval_attn.py")
    tree = ast.parse(open(path).read())
    norm = [n for n in ast.walk(tree) if isinstance(n, ast.Assign) and n.lineno == 21]
    loop = [n for n in ast.walk(tree) if isinstance(n, ast.For) and n.lineno == 31][0]
    record = ast.parse("thr_list.append(t); prec_list.append(prec_ours_t); rec_list.append(rec_ours_t); pp_list.append(int(pred_attn_ours_t.sum())); "
                       "tp_list.append(int((pred_attn_ours_t & (gt_attn != 0)).sum()))").body
    loop.body = [n for n in loop.body if 32 <= n.lineno <= 34] + record
    assert len(norm) == 1 and len(loop.body) == 3 + len(record)
    mod = ast.Module(body=norm + [loop], type_ignores=[])
    return compile(ast.fix_missing_locations(mod), path, "exec")


def flow_code():
    path = os.path.join(shim.REFERENCE_ROOT, "evaluate", "eval_deform.py")
    return _statements(path, lambda n: isinstance(n, ast.Expr) and n.lineno == 18)


def main():
    if not hasattr(np, "bool"):
        np.bool = bool                                                          # eval_attn.py predates numpy 1.24
    arrs, meta = {}, dict(corr_pairs=CORR_PAIRS, attn_meshes=ATTN_MESHES, flow_meshes=FLOW_MESHES, keyframes=KEYFRAMES, margin=MARGIN,
                          numpy=np.__version__)
    # ---- correspondences
    tol_code, body = corr_code()
    ns = {}
    exec(tol_code, ns)
    tolerances = list(ns["ratio_list"])
    assert tolerances == mo.TOLERANCES
    arrs["tolerances"] = np.array(tolerances, dtype=np.float64)
    margin = np.inf
    for b, (n_pts, n_vtx, n_corr) in enumerate(CORR_PAIRS):
        pts, nnind, corr = mo.corr_pair(100 + b, n_pts, n_vtx, n_corr)
        ns = dict(np=np, pts=pts, pred_corr=nnind, gt_corr=corr, ratio_list=tolerances, acc_all=np.zeros(len(tolerances)))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exec(body, ns)
        acc = ns["acc_all"]
        assert ns["dist"].dtype == np.float32
        hits = np.zeros(len(tolerances), dtype=np.int64) if n_corr == 0 else np.rint(acc * n_corr / 100.0).astype(np.int64)
        if n_corr:
            assert np.array_equal(hits / n_corr * 100.0, acc), "the counts do not reproduce the reference's accuracies"
            margin = min(margin, np.abs(ns["dist"].astype(np.float64)[:, None] - np.array(tolerances)[None]).min())
        arrs.update({f"corr_pts{b}": pts, f"corr_nnind{b}": nnind, f"corr_rows{b}": corr, f"corr_acc{b}": acc, f"corr_hits{b}": hits})
    assert margin > MARGIN, margin
    print(f"  correspondences: smallest |dist - tol| {margin:.3e}")
    # ---- attention
    code = attn_code()
    seed, thr_seen, margin = 0, None, np.inf
    for b, n in enumerate(ATTN_MESHES):
        while True:
            seed += 1
            pred, gt = mo.attn_mesh(seed, n)
            ns = dict(np=np, pred_attn_ours=pred.copy(), gt_attn=gt, thr_list=[], prec_list=[], rec_list=[], pp_list=[], tp_list=[])
            exec(code, ns)
            x, thr = ns["pred_attn_ours"], np.array(ns["thr_list"], dtype=np.float64)
            assert x.dtype == np.float32
            inexact = thr[thr.astype(np.float32).astype(np.float64) != thr]
            gap = np.abs(x.astype(np.float64)[:, None] - inexact[None]).min()
            if gap > MARGIN:
                break
        margin = min(margin, gap)
        thr_seen = thr
        arrs.update({f"attn_pred{b}": pred, f"attn_gt{b}": gt, f"attn_precision{b}": np.array(ns["prec_list"], dtype=np.float64),
                     f"attn_recall{b}": np.array(ns["rec_list"], dtype=np.float64), f"attn_pp{b}": np.array(ns["pp_list"], dtype=np.int64),
                     f"attn_tp{b}": np.array(ns["tp_list"], dtype=np.int64), f"attn_gp{b}": np.array(int((gt != 0).sum()), dtype=np.int64)})
    assert np.array_equal(thr_seen, mo.THRESHOLDS)
    arrs["thresholds"] = thr_seen
    print(f"  attention: smallest |x' - t| over the thresholds float32 does not hold exactly {margin:.3e}")
    # ---- key-frame flow
    code = flow_code()
    for b, n in enumerate(FLOW_MESHES):
        rng = np.random.default_rng([0x666C6F77, b])
        gt_flow = rng.normal(0.0, 0.05, (n, 3 * KEYFRAMES)).astype(np.float32)
        pred_flow = (gt_flow + rng.normal(0.0, 0.02, gt_flow.shape)).astype(np.float32)
        diff_t = []
        for t in range(KEYFRAMES):
            exec(code, dict(np=np, diff_t=diff_t, gt_flow_t=gt_flow[:, 3 * t:3 * t + 3], pred_flow_t=pred_flow[:, 3 * t:3 * t + 3]))
        assert len(diff_t) == KEYFRAMES and all(d.dtype == np.float32 for d in diff_t)
        arrs.update({f"flow_pred{b}": pred_flow, f"flow_gt{b}": gt_flow, f"flow_ref{b}": np.asarray(diff_t)})
    msg.save("motion_metrics", meta, **arrs)


if __name__ == "__main__":
    main()
