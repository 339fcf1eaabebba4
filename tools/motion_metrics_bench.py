"""Timing of the motion-stage evaluation (morig_amd/motion_metrics.py) next to the numpy loop a user had to run before (the per-mesh
statements of tests/motion_metrics_oracle.py, one pair / mesh at a time, after copying everything to the host):

    nearest_points + corr_accuracy   --pairs pairs of --vertices vertices x --points points (unit feature rows of width 64) with --corr
                                     correspondences each; the numpy side takes the float32 matrix product and its arg-max per pair
    pr_curve                         --pairs meshes of --vertices vertices
    keyframe_flow_errors             the same meshes, 5 key frames

The device time is wall time around a call that ends in its host read (the tables come to the host, so the call is synchronous), after a
warm-up, median over the repeats; inputs are on the device already, as they are at the end of a forward. The numpy time includes the
device-to-host copies it needs. Counts are compared between the two paths before anything is printed (the arg-max on the rows where the
float64 gap exceeds 1e-4). The shader clock is sampled with ``rocm-smi --showclocks`` after the timed calls. One JSON line; there is NO
threshold: nothing existed before this stage to compare a time with.

    python tools/motion_metrics_bench.py [--pairs 64] [--vertices 4096] [--points 8192] [--corr 2000] [--repeats 7]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_metrics_oracle as mo                 # noqa: E402
from morig_amd import motion_metrics as mm         # noqa: E402


def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def timed(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times) * 1e3, min(times) * 1e3, max(times) * 1e3


def shader_clock():
    try:
        text = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        found = re.findall(r"sclk[^\n]*?\((\d+)\s*Mhz\)", text, flags=re.I)
        return [int(f) for f in found] or "not sampled"
    except Exception:
        return "not sampled"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--corr", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    B, V, P, C, K = a.pairs, a.vertices, a.points, a.corr, 5
    rng = np.random.default_rng(0x6D6F7469)
    pts_f = unit(rng.normal(size=(B * P, 64)))
    target = rng.integers(0, P, B * V) + np.repeat(np.arange(B) * P, V)
    vtx_f = unit(pts_f[target] + 0.05 * rng.normal(size=(B * V, 64)).astype(np.float32))
    pts = rng.random((B * P, 3)).astype(np.float32)
    corr = np.stack([rng.integers(0, V, B * C), rng.integers(0, P, B * C)], 1).astype(np.int64)
    pred = rng.random(B * V).astype(np.float32)
    gt = (rng.random(B * V) < 0.3).astype(np.float32)
    gt_flow = rng.normal(0, 0.05, (B * V, 3 * K)).astype(np.float32)
    pred_flow = (gt_flow + rng.normal(0, 0.02, gt_flow.shape)).astype(np.float32)
    batch = lambda n: np.repeat(np.arange(B, dtype=np.int64), n)
    d = lambda x: torch.from_numpy(x).cuda()
    D = dict(vtx_f=d(vtx_f), pts_f=d(pts_f), pts=d(pts), corr=d(corr), vb=d(batch(V)), pb=d(batch(P)), cb=d(batch(C)), pred=d(pred), gt=d(gt),
             pred_flow=d(pred_flow), gt_flow=d(gt_flow))

    def dev_corr():
        return mm.corr_accuracy(D["pts"], D["corr"], D["pb"], D["cb"], vtx_feature=D["vtx_f"], pts_feature=D["pts_f"], vtx_batch=D["vb"], num_graphs=B)

    def np_corr():
        vf, pf, p, c = D["vtx_f"].cpu().numpy(), D["pts_f"].cpu().numpy(), D["pts"].cpu().numpy(), D["corr"].cpu().numpy()
        pairs = []
        for b in range(B):
            nnind = np.argmax(vf[b * V:(b + 1) * V] @ pf[b * P:(b + 1) * P].T, axis=1)
            pairs.append((p[b * P:(b + 1) * P], nnind, c[b * C:(b + 1) * C]))
        return mo.corr_accuracy(pairs), pairs

    def dev_pr():
        return mm.pr_curve(D["pred"], D["gt"], D["vb"], num_graphs=B)

    def np_pr():
        x, g = D["pred"].cpu().numpy(), D["gt"].cpu().numpy()
        return mo.pr_curve([(x[b * V:(b + 1) * V], g[b * V:(b + 1) * V]) for b in range(B)])

    def dev_flow():
        return mm.keyframe_flow_errors(D["pred_flow"], D["gt_flow"], D["vb"], num_graphs=B)

    def np_flow():
        x, g = D["pred_flow"].cpu().numpy(), D["gt_flow"].cpu().numpy()
        return mo.keyframe_flow_errors([(x[b * V:(b + 1) * V], g[b * V:(b + 1) * V]) for b in range(B)])

    out = dict(pairs=B, vertices=V, points=P, corr=C, keyframes=K, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    got_c, out["corr_device_ms"], lo, hi = timed(dev_corr, a.repeats)
    out["corr_device_ms_range"] = [lo, hi]
    t0 = time.perf_counter()
    want_c, pairs = np_corr()
    out["corr_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    # the arg-max may differ where two similarities are nearly tied: compare the counts with the device's own arg-max on those rows
    local = mm.nearest_points(D["vtx_f"], D["pts_f"], D["vb"], D["pb"], num_graphs=B).cpu().numpy()
    differ = 0
    for b in range(B):
        mine = local[b * V:(b + 1) * V]
        rows = np.nonzero(mine != pairs[b][1])[0]
        differ += len(rows)
        if len(rows):
            assert mo.similarity_gaps(vtx_f[b * V:(b + 1) * V][rows], pts_f[b * P:(b + 1) * P]).max() < 1e-4, "an arg-max differs on a clear row"
        pairs[b] = (pairs[b][0], mine, pairs[b][2])
    assert np.array_equal(got_c["hits"], mo.corr_accuracy(pairs)["hits"]), "corr_accuracy differs from the numpy loop"
    out["argmax_rows_that_differ"] = differ
    got_p, out["pr_device_ms"], lo, hi = timed(dev_pr, a.repeats)
    out["pr_device_ms_range"] = [lo, hi]
    t0 = time.perf_counter()
    want_p = np_pr()
    out["pr_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    assert all(np.array_equal(got_p[k], want_p[k]) for k in ("tp", "pp", "gp", "precision", "recall")), "pr_curve differs from the numpy loop"
    got_f, out["flow_device_ms"], lo, hi = timed(dev_flow, a.repeats)
    out["flow_device_ms_range"] = [lo, hi]
    t0 = time.perf_counter()
    want_f = np_flow()
    out["flow_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    assert np.allclose(got_f[0], want_f[0], rtol=1e-12, atol=0), "keyframe_flow_errors differs from the numpy loop"
    out["sclk_mhz"] = shader_clock()
    out["date"] = time.strftime("%Y-%m-%d")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
